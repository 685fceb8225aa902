"""What the designed flats of tests/flat_fields.py ARE, without a GPU: the regions the reference's labelling finds are the
drawn ones, the host twin equals the numpy statement of the reference bit for bit, and -- from an instrumented copy of
conditioning_numpy._chamfer_distance -- in which sweep each distance of each lake stops and how many cells ONE MORE sweep
would change.  The last number is why tests/test_gpu_flat_engines.py can fail: on every zigzag a region that stops one
sweep late leaves different distances behind.  The stops are pinned as measured (no closed form assumed); the claims
the engine tests rely on (which sweep of which 16-sweep pass, the sizes against the engine thresholds) are asserted
from them."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import conditioning_numpy as CN
import flat_fields as F
from pydem_amd import conditioning as C

ENTRY, T = 33, 16            # the several-sweeps-per-pass engine starts at sweep 33 (after 32 launches per sweep) with 16 sweeps per pass


@functools.lru_cache(maxsize=None)
def fields():
    return {f.name: f for f in F.all_fields()}


NAMES = ['zigzag_k30_v3', 'zigzag_k40_v5', 'zigzag_k30_v4_apart20', 'zig_family', 'default_route', 'long_zigzag', 'edge_lakes', 'centre_seeds']


def test_the_field_list():
    assert list(fields()) == NAMES


def _labels(z):
    flat = (ndimage.minimum_filter(z, (3, 3)) >= z) & (z > 0)
    flat[0, 0] = flat[-1, 0] = flat[0, -1] = flat[-1, -1] = False
    return ndimage.label(flat, structure=np.ones((3, 3), bool))


@pytest.mark.parametrize('name', NAMES)
def test_labelled_regions_are_the_drawn_ones(name):
    f = fields()[name]
    lab, nlab = _labels(f.z)
    assert nlab == len(f.lakes) + len(f.sinks)
    seen = set()
    for lake in f.lakes:
        ids = np.unique(lab[lake.mask])
        assert ids.size == 1 and ids[0] > 0, lake.name
        assert np.array_equal(lab == ids[0], lake.mask), lake.name
        seen.add(int(ids[0]))
    for s in f.sinks:                      # the one-pixel pits beyond the outlets: regions of their own
        assert lab[s] > 0 and (lab == lab[s]).sum() == 1
        seen.add(int(lab[s]))
    assert len(seen) == nlab


@pytest.mark.parametrize('name', NAMES)
def test_host_twin_equals_the_numpy_statement(name):
    z = fields()[name].z
    for elev in (z, z.astype(np.int16)):
        for area in (0.0, 32.0):
            got = C.fill_flats(elev.copy(), area)
            want = CN.fill_flats(elev.copy(), area)
            assert got.dtype == want.dtype == np.float64
            assert np.array_equal(got, want), (name, elev.dtype, area, int((got != want).sum()))
    assert not np.array_equal(C.fill_flats(z.copy(), 0.0), z)


def _one_sweep(d, region):
    straight = ndimage.minimum_filter(d, footprint=CN._CROSS) + 1
    diagonal = ndimage.minimum_filter(d, (3, 3)) + CN._SQRT2
    out = d.copy()
    out[region] = np.minimum(np.minimum(straight[region], diagonal[region]), d[region])
    return out


def _instrumented_chamfer(log, region, seeds):
    """conditioning_numpy._chamfer_distance, sweep for sweep, that also notes the sweep it stopped in and the number of cells
    one more sweep would have changed."""
    big = float(region.size)
    d = np.full(region.shape, big)
    d[seeds] = 0
    stop = 0
    for stop in range(1, region.size + 1):
        d = _one_sweep(d, region)
        if (d[region] < big).all():
            break
    log.append((int(region.sum()), stop, int((_one_sweep(d, region) != d).sum())))
    return d


@functools.lru_cache(maxsize=None)
def stops(name):
    """Per lake, in label (raster) order: (cells, stop of the uphill distance, cells one more sweep changes, stop of the
    outlet distance, cells one more sweep changes).  Also checks that the instrumented copy computes what the original does."""
    z = fields()[name].z
    log = []
    original = CN._chamfer_distance
    CN._chamfer_distance = functools.partial(_instrumented_chamfer, log)
    try:
        out = CN.fill_flats(z.copy(), 0.0)
    finally:
        CN._chamfer_distance = original
    assert np.array_equal(out, CN.fill_flats(z.copy(), 0.0))
    assert len(log) == 2 * len(fields()[name].lakes)
    return tuple((hi[0], hi[1], hi[2], lo[1], lo[2]) for hi, lo in zip(log[0::2], log[1::2]))


PINNED = {
    'zigzag_k30_v3': ((126, 63, 1, 62, 1),),
    'zigzag_k40_v5': ((170, 85, 1, 84, 1),),
    'zigzag_k30_v4_apart20': ((148, 64, 1, 83, 1),),
    'default_route': ((16900, 130, 0, 130, 0), (126, 63, 1, 62, 1), (170, 85, 1, 84, 1), (246, 108, 1, 137, 1)),
    'long_zigzag': ((1058, 529, 1, 528, 1),),
    'edge_lakes': ((945, 45, 0, 44, 0), (987, 47, 0, 46, 0), (945, 45, 0, 44, 0), (756, 36, 0, 35, 0)),
    'centre_seeds': ((5184, 36, 0, 36, 0), (5184, 72, 0, 36, 0)),
    'zig_family': ((68, 34, 1, 33, 1), (74, 37, 1, 36, 1), (90, 40, 1, 49, 1), (82, 41, 1, 40, 1), (88, 44, 1, 43, 1), (88, 44, 1, 43, 1),
                   (108, 48, 1, 59, 1), (100, 50, 1, 49, 1), (100, 50, 1, 49, 1), (110, 55, 1, 54, 1), (110, 55, 1, 54, 1), (136, 58, 1, 77, 1),
                   (116, 58, 1, 57, 1), (122, 61, 1, 60, 1), (126, 63, 1, 62, 1), (134, 67, 1, 66, 1), (136, 68, 1, 67, 1), (165, 70, 1, 94, 1),
                   (142, 71, 1, 70, 1), (154, 77, 1, 76, 1), (160, 80, 1, 79, 1), (170, 85, 1, 84, 1), (216, 93, 1, 122, 1), (198, 99, 1, 98, 1),
                   (9216, 96, 0, 96, 0)),
}


@pytest.mark.parametrize('name', NAMES)
def test_stop_sweeps_are_pinned(name):
    assert stops(name) == PINNED[name]


def lakes_in_label_order(name):
    """scipy numbers the regions by their first cell in raster order; the records of stops() come in that order."""
    return sorted(fields()[name].lakes, key=lambda lake: int(np.flatnonzero(lake.mask)[0]))


def _zigzags():
    for name in NAMES:
        for lake, rec in zip(lakes_in_label_order(name), stops(name)):
            if lake.name.startswith('zig'):
                yield name, lake, rec


def test_one_more_sweep_changes_every_zigzag():
    """The proof that a late stop shows: in every zigzag, for BOTH distances, the sweep after the stopping one changes a cell."""
    n = 0
    for name, lake, (cells, stop_hi, more_hi, stop_lo, more_lo) in _zigzags():
        assert more_hi >= 1 and more_lo >= 1, (name, lake.name)
        n += 1
    assert n == 3 + 24 + 3 + 1
    # ... and on the plain lakes it changes nothing: they cannot see a late stop
    for name in ('default_route', 'zig_family', 'edge_lakes', 'centre_seeds'):
        for lake, rec in zip(lakes_in_label_order(name), stops(name)):
            if not lake.name.startswith('zig'):
                assert rec[2] == 0 and rec[4] == 0, (name, lake.name)


def _pass_and_sweep(stop, entry=ENTRY):
    return (stop - entry) // T, (stop - entry) % T


def test_family_stops_cover_the_sweeps_of_a_pass():
    recs = stops('zig_family')
    all_stops = [s for r in recs[:-1] for s in (r[1], r[3])]
    assert min(all_stops) >= ENTRY                         # nobody has stopped when the engine starts
    js = {_pass_and_sweep(s)[1] for s in all_stops}
    assert 0 in js and T - 1 in js and len(js - {0, T - 1}) >= 8, sorted(js)
    assert len({_pass_and_sweep(s)[0] for s in all_stops}) >= 4      # over several passes: early stoppers lie in the halo of late ones
    assert len(recs) > 8                                   # more regions than PYDEM_FLAT_BATCH_REGIONS=8 has table rows
    assert _pass_and_sweep(recs[-1][1])[0] >= 3            # the plain lake is still sweeping when most zigzags have stopped


def test_family_blocks():
    """One lake has cells in all four 32 x 32 blocks around a block corner; two lakes that stop in different sweeps have cells in
    the same block."""
    f, recs = fields()['zig_family'], stops('zig_family')
    blocks = []
    assert lakes_in_label_order('zig_family')[-1].name == 'ballast'
    for lake in lakes_in_label_order('zig_family'):
        i, j = np.nonzero(lake.mask)
        blocks.append(set(zip((i // 32).tolist(), (j // 32).tolist())))
    assert any({(a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1)} <= bl for bl in blocks[:-1] for a, b in bl)
    assert any(blocks[p] & blocks[q] and recs[p][1] != recs[q][1] for p in range(len(blocks) - 1) for q in range(p))


def test_uphill_and_outlet_distance_stop_in_different_passes():
    assert lakes_in_label_order('default_route')[3].name == 'zig_k52_v4_apart30'
    for name, idx in (('zigzag_k30_v4_apart20', 0), ('default_route', 3)):
        cells, stop_hi, _, stop_lo, _ = stops(name)[idx]
        assert _pass_and_sweep(stop_hi)[0] != _pass_and_sweep(stop_lo)[0], name
    # the long zigzag: uphill stops in the FIRST sweep of a pass, the outlet distance in the LAST sweep of the pass before
    cells, stop_hi, _, stop_lo, _ = stops('long_zigzag')[0]
    assert _pass_and_sweep(stop_hi, 513) == (1, 0) and _pass_and_sweep(stop_lo, 513) == (0, T - 1)
    # mid-pass stops after sweep 33 in default_route
    for rec in stops('default_route')[1:]:
        assert rec[1] > ENTRY and rec[3] > ENTRY and 0 < _pass_and_sweep(rec[1])[1] < T - 1


def _first_list(name):
    """Length of the work list of sweep 1: the cells of the regions that are swept (here: every lake)."""
    return sum(int(lake.mask.sum()) for lake in fields()[name].lakes)


def test_sizes_against_the_engine_thresholds():
    assert _first_list('default_route') > 16384                      # longer than PYDEM_FLAT_BATCH: single sweeps first
    assert _first_list('long_zigzag') <= 8192                        # the resident-workgroup kernel takes it ...
    assert min(stops('long_zigzag')[0][1], stops('long_zigzag')[0][3]) > 513      # ... and its 512 sweeps do not finish it
    assert 8192 < _first_list('zig_family') <= 16384                 # launches per sweep first, with no environment set too
    for name in ('zigzag_k30_v3', 'zigzag_k40_v5', 'zigzag_k30_v4_apart20', 'long_zigzag', 'edge_lakes'):
        assert _first_list(name) <= 4096                             # the one-workgroup kernel takes them (PYDEM_FLAT_COOP=0)
    # the edge and centre-seeded lakes still sweep at 33
    for name in ('edge_lakes', 'centre_seeds'):
        for rec in stops(name):
            assert max(rec[1], rec[3]) > ENTRY, name
    n, m = fields()['edge_lakes'].z.shape
    assert n % 32 and m % 32
    masks = {lake.name: lake.mask for lake in fields()['edge_lakes'].lakes}
    assert masks['bottom'][n - 1].any() and masks['right'][:, m - 1].any() and masks['top'][0].any() and masks['left'][:, 0].any()
    assert (n - 1) // 32 == n // 32 and masks['bottom'][32 * (n // 32):].any() and masks['right'][:, 32 * (m // 32):].any()
