"""The HAND hydraulic table on the device (pydem_hand_table, DEMProcessor.calc_hand_hydraulics / calc_inundation) against its
numpy twin (pydem_amd/hydraulics.py: hand_table_ref).  Everything the device sums is an integer, so every comparison is
np.array_equal and the quanta compare with ==; no tolerance anywhere.

The raw call runs on tiles that only hold a spacing and a slope plane (no flow graph is needed with a HAND plane from the host):
(5, 7) is less than one wavefront, (64, 64) whole wavefronts, (96, 80) and (300, 260) have a last wavefront that is only partly
filled.  Each case runs twice in this process and once in a child under PYDEM_HANDTAB_LOCAL=0 (no reduction across the wavefront)
and PYDEM_MEM_POISON (a table that is not zeroed shows up); the bytes must be the same.  Then the error codes, one tile above
the cap of the grid against the closed form of the wedge, and the pipeline on the tiles of test_gpu_stream_network.py."""
import hashlib
import warnings

import numpy as np
import pytest

from flowgraph_kit import _same_snapshot, _snapshot, fractal_pair as make, nan_speck_pair, run_child
from test_hand_hydraulics_ref import (case, designed_cases, random_case, ref, uniform_case, wedge_case, wedge_closed_form)
from test_stream_network_ref import top_fraction

pytestmark = pytest.mark.gpu

TILES = [((300, 260), 5), ((96, 80), 5)]           # (the tiles of test_gpu_stream_network.py: >= 20 links at the top 5 % of uca)


# ---- the raw call ------------------------------------------------------------------------------------------------------------
def raw_tile(c):
    """a tile that holds what pydem_hand_table reads with a HAND plane from the host: the spacing and the slope"""
    from pydem_amd import _ffi
    n, m = c['zone'].shape
    t = _ffi.Tile(n, m)
    t.set_spacing(c['dX2'][:-1], c['dY2'][:-1], c['dX2'], c['dY2'])
    t.upload(_ffi.MAG, c['mag'])
    return t


def own_zone_case():
    """every cell its own zone: every lane of a wavefront holds another key"""
    n = m = 40
    rng = np.random.default_rng(4)
    return case(np.arange(1, n * m + 1, dtype=np.int32).reshape(n, m), rng.choice([0.25, 1.5, 2.0, 3.5, np.nan], (n, m)), [1.0, 2.0, 3.0])


def stripes_case(shape):
    """one-column zones: distinct keys inside a wavefront, the same keys from every wavefront"""
    n, m = shape
    rng = np.random.default_rng(5)
    return case(np.repeat(np.arange(1, m + 1, dtype=np.int32)[None, :], n, axis=0), rng.uniform(0.0, 3.0, shape), [1.0, 2.0, 3.0])


def raw_cases():
    out = [(name, c) for name, c in designed_cases()]
    out += [('one key %r' % (s,), uniform_case(s)) for s in ((5, 7), (64, 64), (300, 260))]
    out += [('own zone', own_zone_case()), ('stripes (64, 64)', stripes_case((64, 64))), ('stripes (96, 80)', stripes_case((96, 80)))]
    out += [('random %r' % (s,), random_case(s, K, S, seed, per_row=per_row))
            for s, K, S, seed, per_row in (((5, 7), 3, 4, 10, False), ((64, 64), 9, 6, 11, False), ((96, 80), 40, 12, 12, True),
                                           ((300, 260), 500, 32, 13, False))]
    out += [('S = 1', random_case((64, 64), 5, 1, 14)), ('S = 1024', random_case((96, 80), 6, 1024, 15)),
            ('wedge (96, 80)', wedge_case((96, 80), 11, 30))]
    out.append(('K = 0', dict(random_case((64, 64), 4, 3, 16), K=0, zone=np.zeros((64, 64), np.int32) - np.eye(64, dtype=np.int32))))
    return out


def check_raw_cases():
    """every raw case against the twin, twice; returns the sha256 over all the device's words"""
    sha = hashlib.sha256()
    for name, c in raw_cases():
        want_ints, want_skipped, want_quanta = ref(c)
        t = raw_tile(c)
        for k in range(2):
            ints, skipped, quanta, ms = t.hand_table(c['zone'], c['stages'], c['K'], hand=c['hand'])
            assert ints.dtype == np.int64 and ints.shape == want_ints.shape and skipped.shape == want_skipped.shape, name
            bad = ints != want_ints
            assert not bad.any(), "%s, call %d: %d words differ, first (zone, bin, word) %r" % (name, k, bad.sum(), np.argwhere(bad)[0].tolist())
            assert np.array_equal(skipped, want_skipped), name
            assert quanta == want_quanta, (name, quanta, want_quanta)
            assert set(ms) == {'total', 'maxima', 'sums'} and ms['maxima'] > 0 and ms['total'] == ms['maxima'] + ms['sums']
            sha.update(ints.tobytes()); sha.update(skipped.tobytes()); sha.update(np.asarray(quanta).tobytes())
        t.close()
    return sha.hexdigest()


def test_raw_call_equals_the_twin_under_both_schedules():
    here = check_raw_cases()
    r = run_child("from test_gpu_hand_hydraulics import check_raw_cases\nprint('BITS', check_raw_cases())\nprint('CHILD-OK')",
                  env={'PYDEM_HANDTAB_LOCAL': '0', 'PYDEM_MEM_POISON': '0xA5'}, timeout=300)
    there = r.stdout.split('BITS', 1)[1].split()[0]
    assert there == here


def test_cases_cover_what_they_are_meant_to():
    cases = dict(raw_cases())
    c = cases['own zone']
    assert c['K'] == 1600 and np.unique(c['zone']).size == 1600
    c = cases['random (300, 260)']
    ints, skipped, _ = ref(c)
    assert np.isnan(c['hand']).mean() > 0.08 and (c['zone'] < 1).any() and skipped.all(axis=0).all()
    assert (ints[:, :, 0].sum(axis=0) > 0).all()                         # every bin is filled
    assert ref(cases['S = 1024'])[0].shape == (6, 1024, 4) and (ref(cases['S = 1024'])[0][:, :, 0].sum(axis=0) > 0).sum() > 500
    assert np.ptp(cases['random (96, 80)']['dX2']) > 0                    # per-row spacing


def test_error_codes():
    from pydem_amd import _ffi
    c = random_case((64, 64), 5, 4, 20)
    t = raw_tile(c)
    call = lambda **kw: t.hand_table(kw.get('zone', c['zone']), kw.get('stages', c['stages']), kw.get('K', c['K']), hand=kw.get('hand', c['hand']))
    for stages in ([], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf], [-np.inf, 0.0], np.arange(1025.0)):
        with pytest.raises(_ffi.HipError, match='error -2'):
            call(stages=stages)
    with pytest.raises(_ffi.HipError, match='error -2'):
        call(K=4)                                                       # the plane holds zone 5
    with pytest.raises(_ffi.HipError, match='error -2'):
        call(K=-1)
    bad = c['hand'].copy()
    bad[c['zone'] == 1] = -np.inf
    with pytest.raises(_ffi.HipError, match='error -2'):
        call(hand=bad)
    with pytest.raises(_ffi.HipError, match='error -3'):
        call(hand=None)                                                 # no dist_down result on this tile
    with pytest.raises(ValueError):
        call(zone=c['zone'][:, :-1])
    with pytest.raises(ValueError):
        call(hand=c['hand'][:-1])
    bare = _ffi.Tile(64, 64)
    with pytest.raises(_ffi.HipError, match='error -3'):                # no spacing, no slope
        bare.hand_table(c['zone'], c['stages'], c['K'], hand=c['hand'])
    bare.set_spacing(c['dX2'][:-1], c['dY2'][:-1], c['dX2'], c['dY2'])
    with pytest.raises(_ffi.HipError, match='error -3'):
        bare.hand_table(c['zone'], c['stages'], c['K'], hand=c['hand'])
    # ... and the tile still works after all of them
    want = ref(c)
    got = call()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_resident_tag():
    """hand=None reads the result plane of pydem_dist_down only while it holds one"""
    from pydem_amd import _ffi
    shape, seed = TILES[1]
    o, dp = make(shape, seed)                           # (a pair of this test's own)
    tile = dp._tile
    thr = top_fraction(dp.uca, 0.05)
    zone = np.ones(shape, np.int32)
    stages = [1.0, 5.0, 25.0]
    resident = lambda: tile.hand_table(zone, stages, 1, hand=None)
    with pytest.raises(_ffi.HipError, match='error -3'):
        resident()                                                      # a flow graph, no sweep yet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hand, _, _, _ = tile.dist_down('v', 'ave', None, thr)
        first = resident()
        host = tile.hand_table(zone, stages, 1, hand=hand)
        assert all(np.array_equal(a, b) for a, b in zip(first[:2], host[:2])) and first[2] == host[2]
        assert first[0][0, :, 0].sum() > 0
        assert resident()[0].tobytes() == first[0].tobytes()            # the call itself leaves the tag alone
        for spoil in (lambda: tile.dist_up('h', 'max', True, download=False),
                      lambda: tile.rev_accum('sum', None, zone, 1.0, download=False),
                      lambda: tile.stream_network(None, thr),
                      lambda: tile.upload(_ffi.ELEV, np.asarray(o.elev, np.float64))):
            tile.dist_down('v', 'ave', None, thr, download=False)
            assert resident()[0].tobytes() == first[0].tobytes()
            spoil()
            with pytest.raises(_ffi.HipError, match='error -3'):
                resident()
    # the upload dropped the flow graph too: the plane is stale until a new sweep on a new graph
    with pytest.raises(_ffi.HipError, match='error -3'):
        resident()


# ---- above the cap of the grid -----------------------------------------------------------------------------------------------
def test_wedge_above_the_grid_cap():
    """8192 workgroups of 256 lanes cover 2 097 152 cells per stride: 2100 x 2100 needs three strides, the last one partial"""
    from pydem_amd import hydraulics as H
    shape, band, c0 = (2100, 2100), 173, 1000
    assert shape[0] * shape[1] > 2 * 8192 * 256
    c = wedge_case(shape, band, c0)
    t = raw_tile(c)
    ints, skipped, quanta, _ = t.hand_table(c['zone'], c['stages'], c['K'], hand=c['hand'])
    t.close()
    tab = H.hydraulic_table(ints, quanta, c['stages'], np.ones(c['K']), np.ones(c['K']), 0.05)
    cells, area, volume, above = wedge_closed_form(shape, band, c0)
    assert np.array_equal(tab['cells'], cells) and np.array_equal(tab['area'], area) and np.array_equal(tab['volume'], volume)
    assert np.array_equal(tab['bed_area'], 1.25 * area)
    assert np.array_equal(skipped[:, 1], above) and not skipped[:, 0].any()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def pipeline(dp, thr):
    """calc_hand_hydraulics with stages at the 10 / 30 / 50 / 70 / 90 % quantiles of the tile's finite HAND: (result, stages,
    HAND, the resident slope)"""
    from pydem_amd import _ffi
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hand = np.array(dp.calc_hand(uca_threshold=thr))
        stages = np.quantile(hand[np.isfinite(hand)], [0.1, 0.3, 0.5, 0.7, 0.9])
        assert (np.diff(stages) > 0).all()
        hh = dp.calc_hand_hydraulics(stages, uca_threshold=thr)
    return hh, stages, hand, dp._tile.download(_ffi.MAG)


@pytest.mark.parametrize('shape,seed', TILES)
def test_pipeline(shape, seed):
    from pydem_amd import hydraulics as H
    o, dp = make(shape, seed)                           # (a pair of this test's own: the test uploads nothing, but it asks for state)
    thr = top_fraction(dp.uca, 0.05)
    hh, stages, hand, mag = pipeline(dp, thr)
    net, reaches = dp.stream_network, dp.reach_attributes
    K = net.links.size
    assert hh is dp.hand_hydraulics and K >= 20 and net.basin is hh.zone and np.array_equal(hh.link_ids, net.links['id'])
    # the integers are the twin's on the host copies of the same planes
    want_ints, want_skipped, want_quanta = H.hand_table_ref(net.basin, hand, stages, dp.dX2, dp.dY2, mag, K)
    assert (want_ints[:, :, 0].sum(axis=0) > 0).all() and want_skipped[:, 1].sum() > 0      # every bin is filled, and the top is passed
    assert np.array_equal(hh.ints, want_ints) and np.array_equal(hh.skipped, want_skipped) and hh.quanta == want_quanta
    assert np.array_equal(hh.cells_nan, want_skipped[:, 0]) and np.array_equal(hh.cells_above, want_skipped[:, 1])
    # resident plane and host plane: the same bytes (calc_hand_hydraulics left its HAND on the device)
    tile = dp._tile
    res = tile.hand_table(net.basin, stages, K, hand=None)
    host = tile.hand_table(net.basin, stages, K, hand=hand)
    for got in (res, host):
        assert got[0].tobytes() == want_ints.tobytes() and got[1].tobytes() == want_skipped.tobytes() and got[2] == want_quanta
    # conservation per link
    basin = net.basin.ravel()
    assert np.array_equal(hh.ints[:, :, 0].sum(axis=1) + hh.skipped.sum(axis=1), np.bincount(basin[basin >= 1], minlength=K + 1)[1:])
    # the table
    want = H.hydraulic_table(want_ints, want_quanta, stages, reaches['length'], reaches['slope'], 0.05)
    for k in H.TABLE_COLUMNS:
        assert np.array_equal(getattr(hh, k), want[k], equal_nan=True), k
    assert np.array_equal(hh.length, reaches['length']) and np.array_equal(hh.slope, reaches['slope'], equal_nan=True)
    for k in ('cells', 'area', 'bed_area'):
        assert (np.diff(getattr(hh, k), axis=1) >= 0).all(), k
    with np.errstate(invalid='ignore'):
        nonneg = np.ones(K, bool)
        nonneg[basin[(basin >= 1) & (hand.ravel() < 0)] - 1] = False
    print("%r: %d links, %d with h >= 0 throughout" % (shape, K, nonneg.sum()))
    assert nonneg.any() and (np.diff(hh.volume[nonneg], axis=1) >= 0).all()
    assert (hh.bed_area >= hh.area).all()               # (a = 900 is a multiple of both quanta: no rounding can invert it)
    assert np.isfinite(hh.discharge).any()
    st = dp.hand_hydraulics_stats
    assert st['n_links'] == K and st['n_stages'] == 5 and set(st['ms']) >= {'reach_attributes', 'stream_network', 'dist_down', 'hand_table'}
    assert all(v > 0 for v in st['ms'].values())


def test_state_integrity_and_repeats():
    shape, seed = TILES[1]
    o, dp = make(shape, seed)
    thr = top_fraction(dp.uca, 0.05)
    hh, stages, hand, _ = pipeline(dp, thr)
    tile, zone, K = dp._tile, dp.stream_network.basin, dp.stream_network.links.size
    before, bytes_before = _snapshot(dp), tile.device_bytes()
    first = tile.hand_table(zone, stages, K, hand=None)
    for k in range(6):
        got = tile.hand_table(zone, stages, K, hand=None if k % 2 else hand)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes() and got[2] == first[2]
    _same_snapshot(before, _snapshot(dp))
    assert tile.device_bytes() == bytes_before
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        again = dp.calc_hand_hydraulics(stages, uca_threshold=thr)
        assert np.array(dp.calc_hand(uca_threshold=thr)).tobytes() == hand.tobytes()
    assert again.ints.tobytes() == hh.ints.tobytes() and again.skipped.tobytes() == hh.skipped.tobytes() and again.quanta == hh.quanta
    assert all(np.array_equal(getattr(again, k), getattr(hh, k), equal_nan=True) for k in ('discharge', 'volume', 'area'))


def test_nan_specks_are_counted():
    n, m = 96, 80
    z, _, dp, _ = nan_speck_pair((n, m), 12, [(0, 5), (95, 30), (20, 0)])
    hh, stages, hand, _ = pipeline(dp, 50 * 900.0)
    assert hh.cells_nan.sum() > 0 and hh.link_ids.size >= 20
    basin = dp.stream_network.basin
    assert hh.cells_nan.sum() == (np.isnan(hand) & (basin >= 1)).sum()
    assert (basin[np.isnan(z)] < 1).all()               # a no-data cell belongs to no basin


def _depth(hand, basin, level):
    """the formula of calc_inundation, spelled out"""
    out = np.full(hand.shape, np.nan)
    inside = basin >= 1
    with np.errstate(invalid='ignore'):
        out[inside] = np.maximum(level[basin[inside] - 1] - hand[inside], 0.0)
    out[np.isnan(hand)] = np.nan
    return out


def test_inundation():
    shape, seed = TILES[1]
    o, dp = make(shape, seed)
    thr = top_fraction(dp.uca, 0.05)
    hh, stages, hand, _ = pipeline(dp, thr)
    basin, K = dp.stream_network.basin, hh.link_ids.size
    nowhere = np.isnan(hand) | (basin < 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        depth = dp.calc_inundation(stage=float(stages[2]))
        assert depth is dp.inundation and dp.hand.tobytes() == hand.tobytes()
        assert np.array_equal(np.isnan(depth), nowhere)                 # NaN exactly where HAND is NaN or the cell has no basin
        assert np.array_equal(depth, _depth(hand, basin, np.full(K, stages[2])), equal_nan=True)
        assert (depth[~nowhere] >= 0).all() and (depth[~nowhere] > 0).any() and (depth[~nowhere] == 0).any()
        levels = np.random.default_rng(8).uniform(stages[0], stages[-1], K)
        assert np.array_equal(dp.calc_inundation(stage=levels), _depth(hand, basin, levels), equal_nan=True)
        # a discharge read back from the table, and one between two of its points
        for q in (hh.discharge[:, 3], 0.5 * (hh.discharge[:, 1] + hh.discharge[:, 3])):
            want = np.full(K, np.nan)
            for k in range(K):
                ok = np.isfinite(hh.discharge[k])
                if ok.any() and not np.isnan(q[k]) and (np.diff(hh.discharge[k][ok]) >= 0).all():
                    want[k] = np.interp(q[k], hh.discharge[k][ok], stages[ok], right=np.nan)
            print("%d of %d links have a stage for their discharge" % (np.isfinite(want).sum(), K))
            assert np.isfinite(want).any()
            got = dp.calc_inundation(discharge=q)
            assert np.array_equal(got, _depth(hand, basin, want), equal_nan=True)
            assert not np.isnan(got[~nowhere & np.isfinite(want)[np.maximum(basin, 1) - 1]]).any()
