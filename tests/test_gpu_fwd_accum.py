"""Decaying and transport-limited accumulation on the device (DEMProcessor.calc_decay_accum / calc_trans_lim_accum,
pydem_fwd_accum) against the forward Kahn reference of tests/test_fwd_accum_ref.py on the oracle's graphs, cell by cell:

    NaN patterns identical, |dev - ref| <= 1e-9 * refabs   for the value V, the inflow I and the deposition D

(refabs: the same recursion with |load|, |mult| and no cap; 1e-9 is the project's bound for sums on this graph), in the form of
tests/test_gpu_dist_up.py.  Then the designed flow fields of tests/flow_fields.py, the schedules (bit-identical), what the call
must leave alone, run-to-run identity, the memory it holds and its error codes."""
import functools
import warnings

import numpy as np
import pytest

from flowgraph_kit import (_same_snapshot, _snapshot, assert_bound, bits, circular_case, nan_speck_pair, pair, random_weights, run_child,
                           shared_deep_pair as deep_pair, shared_fractal_pair as fractal_pair)
from test_dist_up_ref import edge_nan_cells
from test_fwd_accum_ref import fwd_accum_ref

pytestmark = pytest.mark.gpu

BOUND = 1e-9            # (no floor: where refabs is 0 the device must give the reference's value)
REFS = {}               # key -> (reference, reference on absolute values): computed once, shared, never written to


def reference(o, load, mult, cap, edge_nan, key=None):
    if key is None or key not in REFS:
        res = fwd_accum_ref(o, load, mult, cap, edge_nan), fwd_accum_ref(o, load, mult, cap, edge_nan, absolute=True)
        if key is None:
            return res
        REFS[key] = res
    return REFS[key]


def compare(dev_v, dev_i, o, load, mult, cap, edge_nan, what, key=None, min_finite=None):
    """the device's V (and I, and the deposition they give, when dev_i is not None) against the reference: (V, I, final, depth)"""
    (V, I, final, depth), (Va, Ia, _, _) = reference(o, load, mult, cap, edge_nan, key)
    finite = float(np.isfinite(V).mean())
    print("%s: depth %d, %d cells not final" % (what, depth, (~final).sum()))
    if min_finite is not None:
        assert finite >= min_finite, "%s: only %.1f %% of the reference is finite" % (what, 100 * finite)
    assert_bound(dev_v, V, Va, what + ' V', BOUND)
    if dev_i is not None:
        assert_bound(dev_i, I, Ia, what + ' I', BOUND)
        ld = np.broadcast_to(np.asarray(load, np.float64), V.shape)
        with np.errstate(invalid='ignore'):
            assert_bound((ld + dev_i) - dev_v, (ld + I) - V, Va, what + ' D', BOUND)
    return V, I, final, depth


FRACTALS = [((300, 260), 5), ((700, 520), 41)]


def loads(shape, seed):
    """(signed load, mult in [0.5, 1], supply >= 0) of a tile"""
    rng = np.random.default_rng(seed + 100)
    return random_weights(shape, seed), rng.uniform(0.5, 1.0, shape), rng.uniform(0.0, 2.0, shape)


def assert_deposition(T, D, cap):
    """never negative, exactly 0 wherever the capacity does not bind, and the transport is the capacity wherever it does"""
    ok = np.isfinite(T)
    cap = np.broadcast_to(np.asarray(cap, np.float64), T.shape)
    assert np.array_equal(np.isnan(D), ~ok)
    assert (D[ok] >= 0).all() and (D[ok & (T < cap)] == 0).all() and (T[ok] <= cap[ok]).all()
    with np.errstate(invalid='ignore'):
        assert (T[D > 0] == cap[D > 0]).all()


# ---- 1. fractal tiles
@pytest.mark.parametrize('edge_nan', [True, False])
@pytest.mark.parametrize('shape,seed', FRACTALS)
def test_fractal_tiles_decay(shape, seed, edge_nan):
    o, dp = fractal_pair(shape, seed)
    w, k, _ = loads(shape, seed)
    v = dp.calc_decay_accum(w, edge_nan=edge_nan)
    assert v is dp.decay_accum and v.dtype == np.float64 and v.shape == shape
    _, _, final, depth = compare(v, None, o, w, None, None, edge_nan, 'plain %r edge_nan=%r' % (shape, edge_nan),
                                 key=(shape, 'plain', edge_nan), min_finite=0.7 if edge_nan else 1.0)
    st = dp.decay_accum_stats
    assert set(st) == {'ms', 'levels', 'n_unresolved', 'edge_nan'}
    assert st['n_unresolved'] == (~final).sum() == 0 and 2 <= st['levels'] <= depth and st['ms'] > 0 and st['edge_nan'] == edge_nan
    if not edge_nan:
        assert np.array_equal(np.isfinite(v), np.isfinite(o.elev))
    v = dp.calc_decay_accum(w, decay=k, edge_nan=edge_nan)
    _, _, final, depth = compare(v, None, o, w, k, None, edge_nan, 'decay %r edge_nan=%r' % (shape, edge_nan),
                                 key=(shape, 'decay', edge_nan), min_finite=0.7 if edge_nan else 1.0)
    st = dp.decay_accum_stats
    assert st['n_unresolved'] == 0 and 2 <= st['levels'] <= depth
    # the neutral decay is the call without one, bit for bit
    assert dp.calc_decay_accum(w, decay=1.0, edge_nan=edge_nan).tobytes() == dp.calc_decay_accum(w, edge_nan=edge_nan).tobytes()


@pytest.mark.parametrize('edge_nan', [True, False])
@pytest.mark.parametrize('shape,seed', FRACTALS)
def test_fractal_tiles_trans_lim(shape, seed, edge_nan):
    o, dp = fractal_pair(shape, seed)
    free = reference(o, 1.0, None, None, False, key=(shape, 'count'))[0][0]
    rand = 2.0 * np.median(free) * np.random.default_rng(13).uniform(0.5, 1.5, shape)
    for name, supply, cap, min_capped in (('cap 5', 1.0, 5.0, 0.15), ('random cap', 1.0, rand, 0.15), ('random supply', loads(shape, seed)[2], 3.0, 0.05)):
        T, D = dp.calc_trans_lim_accum(supply, cap, edge_nan=edge_nan)
        assert T is dp.trans_lim_accum and D is dp.trans_lim_deposition and T.shape == D.shape == shape
        what = '%s %r edge_nan=%r' % (name, shape, edge_nan)
        # (the deposition the call returns is the one compare() forms from the device's inflow plane)
        out, flow, _, _, _ = dp._tile.fwd_accum(np.broadcast_to(np.float64(supply), shape), None, np.broadcast_to(np.float64(cap), shape),
                                                edge_nan, inflow=True)
        assert out.tobytes() == T.tobytes()
        with np.errstate(invalid='ignore'):
            assert ((np.broadcast_to(np.float64(supply), shape) + flow) - out).tobytes() == D.tobytes()
        _, I, final, depth = compare(T, flow, o, supply, None, cap, edge_nan, what, key=(shape, name, edge_nan), min_finite=0.7 if edge_nan else 1.0)
        assert_deposition(T, D, cap)
        capped = float(np.mean(D[np.isfinite(D)] > 0))
        print("%s: %.3f of the finite cells deposit" % (what, capped))
        assert capped >= min_capped
        st = dp.trans_lim_stats
        assert set(st) == {'ms', 'levels', 'n_unresolved', 'edge_nan'}
        assert st['n_unresolved'] == (~final).sum() == 0 and 2 <= st['levels'] <= depth and st['ms'] > 0
    # the neutral capacity is the plain accumulation, bit for bit, and deposits nothing
    T, D = dp.calc_trans_lim_accum(1.0, np.inf, edge_nan=edge_nan)
    assert T.tobytes() == dp.calc_decay_accum(1.0, edge_nan=edge_nan).tobytes() and (D[np.isfinite(D)] == 0).all()


# ---- 2. small ramps
@pytest.mark.parametrize('shape', [(3, 7), (7, 3), (31, 33), (33, 65)])
def test_small_ramps(shape):
    """tiles smaller than one 32 x 32 block, and one cell more than a block in each direction"""
    n, m = shape
    z = -np.tile(np.arange(m, dtype=np.float64), (n, 1)) + 0.01 * np.arange(n, dtype=np.float64)[:, None]
    o, dp = pair(z, dX=2.0, dY=3.0)
    w = np.linspace(-1.0, 2.0, n * m).reshape(n, m)
    for edge_nan in (False, True):
        v = dp.calc_decay_accum(w, decay=0.75, edge_nan=edge_nan)
        _, _, final, depth = compare(v, None, o, w, 0.75, None, edge_nan, 'ramp %r decay edge_nan=%r' % (shape, edge_nan))
        assert final.all() and dp.decay_accum_stats['n_unresolved'] == 0 and 1 <= dp.decay_accum_stats['levels'] <= depth
        T, D = dp.calc_trans_lim_accum(1.0, 2.5, edge_nan=edge_nan)
        flow = dp._tile.fwd_accum(np.ones(shape), None, np.full(shape, 2.5), edge_nan, inflow=True)[1]
        compare(T, flow, o, 1.0, None, 2.5, edge_nan, 'ramp %r cap edge_nan=%r' % (shape, edge_nan))
        assert_deposition(T, D, 2.5)
        if edge_nan:
            assert np.isnan(v[0]).all() and np.isnan(v[-1]).all() and np.isnan(v[:, 0]).all() and np.isnan(v[:, -1]).all()
        else:
            assert np.isfinite(v).all() and np.isfinite(T).all() and T.max() == 2.5 and (D > 0).any()


# ---- 3. NaN specks
def test_nan_specks():
    n, m = 200, 230
    z, o, dp, _ = nan_speck_pair((n, m), 40, [(0, 5), (n - 1, 100), (60, 0)])
    assert np.isnan(np.asarray(dp.uca)).any()
    w, k, s = loads((n, m), 3)
    for edge_nan in (False, True):
        v = dp.calc_decay_accum(w, decay=k, edge_nan=edge_nan)
        compare(v, None, o, w, k, None, edge_nan, 'NaN specks decay edge_nan=%r' % edge_nan, min_finite=0.3)
        T, D = dp.calc_trans_lim_accum(s, 4.0, edge_nan=edge_nan)
        flow = dp._tile.fwd_accum(s, None, np.full((n, m), 4.0), edge_nan, inflow=True)[1]
        compare(T, flow, o, s, None, 4.0, edge_nan, 'NaN specks cap edge_nan=%r' % edge_nan, min_finite=0.3)
        assert_deposition(T, D, 4.0)
        for a in (v, T, D, flow):
            assert np.isnan(a[np.isnan(z)]).all()
            if edge_nan:
                assert np.isnan(a[edge_nan_cells(z)]).all()
            else:
                assert np.array_equal(np.isnan(a), np.isnan(z))


# ---- 4. circular drainage
@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_nan_and_counted(loop):
    o, dp = circular_case(loop)
    n, m = dp.shape
    indptr, indices, _ = o.A
    src = np.repeat(np.arange(n * m), np.diff(indptr))
    w = np.linspace(-1.0, 2.0, n * m).reshape(n, m)
    for edge_nan in (False, True):
        with pytest.warns(UserWarning, match='circular drainage'):
            v = dp.calc_decay_accum(w, decay=0.5, edge_nan=edge_nan)
        _, _, final, _ = compare(v, None, o, w, 0.5, None, edge_nan, '%s decay edge_nan=%r' % (loop, edge_nan))
        assert (~final).sum() >= 2 and dp.decay_accum_stats['n_unresolved'] == (~final).sum()
        with pytest.warns(UserWarning, match='circular drainage'):
            T, D = dp.calc_trans_lim_accum(1.0, 3.0, edge_nan=edge_nan)
        flow = dp._tile.fwd_accum(np.ones((n, m)), None, np.full((n, m), 3.0), edge_nan, inflow=True)[1]
        _, _, final, _ = compare(T, flow, o, 1.0, None, 3.0, edge_nan, '%s cap edge_nan=%r' % (loop, edge_nan))
        assert dp.trans_lim_stats['n_unresolved'] == (~final).sum() >= 2
        for a in (v, T, D, flow):
            assert np.isnan(a[~final]).all()
            # the loop cells and everything downstream: NaN flows along every edge, a finite capacity or not
            assert np.isnan(a.ravel()[indices[np.isnan(a.ravel()[src])]]).all()
        if not edge_nan:
            assert np.isfinite(v[final]).all() and np.isfinite(T[final]).all()


# ---- 5. deep ramp
@functools.lru_cache(maxsize=None)
def deep_ramp_depth():
    return fwd_accum_ref(deep_pair()[0], 1.0)[3]


def test_deep_ramp():
    """a 900-row ramp: the forward depth is the tile's length, not a hillslope's"""
    o, dp = deep_pair()
    shape = tuple(dp.shape)
    w, k, _ = loads(shape, 1)
    v = dp.calc_decay_accum(w, decay=k, edge_nan=False)
    _, _, final, depth = compare(v, None, o, w, k, None, False, 'deep ramp decay', min_finite=1.0)
    assert final.all() and depth >= 900 and depth == deep_ramp_depth()
    st = dp.decay_accum_stats
    assert 100 <= st['levels'] <= depth and st['n_unresolved'] == 0
    T, D = dp.calc_trans_lim_accum(1.0, 40.0, edge_nan=False)
    flow = dp._tile.fwd_accum(np.ones(shape), None, np.full(shape, 40.0), False, inflow=True)[1]
    Tr, Ir, _, _ = compare(T, flow, o, 1.0, None, 40.0, False, 'deep ramp cap', min_finite=1.0)
    assert_deposition(T, D, 40.0)
    assert 0.05 < np.mean((1.0 + Ir) - Tr > 0) < 1.0 and (D > 0).any()       # (of the reference: the capacity binds on a part of the ramp)


# ---- 6. the designed flow fields (tests/flow_fields.py, by way of tests/test_gpu_flow_fields.py)
FIELD_NAMES = (['row_snake', 'tile_snake'] + ['fan%d' % k for k in range(8)] + ['far_pit', 'far_pit_rows', 'near_pit', 'tall', 'wide'])
SNAKES = ('row_snake', 'tile_snake', 'tall', 'wide')


def field_pair(name):
    from test_gpu_flow_fields import pair
    return pair(name)


def field_cap(o, name):
    """a capacity that binds on part of every long flow path: the 0.7 quantile of the uncapped count of upslope cells, varied
    by +-25 % from cell to cell"""
    free = reference(o, 1.0, None, None, False, key=(name, 'count'))[0][0]
    assert np.isfinite(free).all()
    q = float(np.quantile(free, 0.7))
    assert 1.0 < q < free.max()
    return q * np.random.default_rng(17).uniform(0.75, 1.25, free.shape)


@pytest.mark.parametrize('edge_nan', [False, True])
@pytest.mark.parametrize('name', FIELD_NAMES)
def test_designed_fields_cell_by_cell(name, edge_nan):
    from test_gpu_flow_fields import weights
    o, dp = field_pair(name)
    shape = tuple(dp.shape)
    w = weights(name)
    k = np.random.default_rng(5).uniform(0.5, 1.0, shape)
    v = dp.calc_decay_accum(w, decay=k, edge_nan=edge_nan)
    _, _, final, depth = compare(v, None, o, w, k, None, edge_nan, '%s decay edge_nan=%r' % (name, edge_nan), key=(name, 'decay', edge_nan),
                                 min_finite=None if edge_nan else 1.0)
    st = dp.decay_accum_stats
    assert final.all() and st['n_unresolved'] == 0 and 1 <= st['levels'] <= depth
    cap = field_cap(o, name)
    T, D = dp.calc_trans_lim_accum(1.0, cap, edge_nan=edge_nan)
    flow = dp._tile.fwd_accum(np.ones(shape), None, cap, edge_nan, inflow=True)[1]
    compare(T, flow, o, 1.0, None, cap, edge_nan, '%s cap edge_nan=%r' % (name, edge_nan), key=(name, 'cap', edge_nan))
    assert_deposition(T, D, cap)
    if not edge_nan:
        assert (D > 0).sum() >= 20 and np.mean(D > 0) < 0.9, np.mean(D > 0)   # the capacity binds on a part of the field
    assert dp.trans_lim_stats['n_unresolved'] == 0


@pytest.mark.parametrize('name', SNAKES)
def test_closed_forms_on_the_chains(name):
    from test_flow_fields import chain_index
    from test_gpu_flow_fields import FIELDS
    field = FIELDS[name]()
    _, dp = field_pair(name)
    to_end, _ = chain_index(field)
    pos = np.zeros(field.elev.shape)                                     # cells from the chain's head, the cell itself included
    for p in field.facts['paths']:
        pos[p[:, 0], p[:, 1]] = 1.0 + np.arange(len(p))
    count = dp.calc_decay_accum(1.0, edge_nan=False)
    assert np.array_equal(count, pos), "%d cells do not hold the count of cells from their chain's head" % (count != pos).sum()
    assert np.array_equal(count + to_end, pos + to_end) and (pos + to_end).max() == 1.0 + field.facts['depth']
    half = dp.calc_decay_accum(1.0, decay=0.5, edge_nan=False)
    assert np.array_equal(half, 2.0 - 0.5 ** (pos - 1.0))                # (exact: 2 - 2^-(pos - 1) until it rounds to 2)
    geo = dp.calc_decay_accum(1.0, decay=0.9, edge_nan=False)
    want = (1.0 - 0.9 ** pos) / (1.0 - 0.9)
    assert (np.abs(geo - want) <= 1e-9 * want).all()
    T, D = dp.calc_trans_lim_accum(1.0, 100.0, edge_nan=False)
    assert np.array_equal(T, np.minimum(pos, 100.0)) and np.array_equal(D, (pos > 100.0).astype(np.float64))
    T, D = dp.calc_trans_lim_accum(1.0, 0.0, edge_nan=False)
    assert (T == 0.0).all() and (D == 1.0).all()


@pytest.mark.parametrize('k', range(8))
def test_fans_agree_with_their_mirror_image(k):
    """a weight given to the wrong neighbour breaks this even if the reference shared the mistake"""
    from test_gpu_flow_fields import weights
    o, dp = field_pair('fan%d' % k)
    _, dpm = field_pair('fan%d_mirror' % k)
    w = weights('fan%d' % k, 11)
    wm = np.ascontiguousarray(w[:, ::-1])
    mult = np.random.default_rng(6).uniform(0.5, 1.0, w.shape)
    multm = np.ascontiguousarray(mult[:, ::-1])
    refabs = reference(o, w, mult, None, False, key=('fan%d' % k, 'mirror'))[1][0]
    a = dp.calc_decay_accum(w, decay=mult, edge_nan=False)
    b = dpm.calc_decay_accum(wm, decay=multm, edge_nan=False)
    assert np.isfinite(a).all() and np.abs(a).max() > 2
    floor = 1e-300                     # (the mirror images are held with the floor of test_gpu_rev_accum's comparisons)
    assert_bound(a, b[:, ::-1], refabs, 'fan%d against its mirror image, decay' % k, BOUND, floor)
    cap = field_cap(o, 'fan%d' % k)
    Ta, Da = dp.calc_trans_lim_accum(1.0, cap, edge_nan=False)
    Tb, Db = dpm.calc_trans_lim_accum(1.0, np.ascontiguousarray(cap[:, ::-1]), edge_nan=False)
    count = reference(o, 1.0, None, None, False, key=('fan%d' % k, 'count'))[0][0]
    assert_bound(Ta, Tb[:, ::-1], count, 'fan%d against its mirror image, transport' % k, BOUND, floor)
    assert_bound(Da, Db[:, ::-1], count, 'fan%d against its mirror image, deposition' % k, BOUND, floor)


# ---- 7. schedules
def schedule_results():
    """what the three schedules must agree on, bit for bit: (case, sha256 of V, sha256 of I, levels, unresolved) per call"""
    import sys
    out = []
    for name, dp in (('fractal', fractal_pair(*FRACTALS[0])[1]), ('deep ramp', deep_pair()[1]), ('two_loops', circular_case('two_loops')[1])):
        shape = tuple(dp.shape)
        w, k, s = loads(shape, 2)
        cap = np.full(shape, 3.0)
        for load, mult, c, edge_nan in ((w, None, None, True), (w, k, None, False), (s, None, cap, True), (s, k, cap, False)):
            if name == 'deep ramp':
                edge_nan = False
            sys.stderr.write('--- %s\n' % name)
            sys.stderr.flush()
            v, flow, _, levels, left = dp._tile.fwd_accum(load, mult, c, edge_nan, inflow=True)
            out.append((name, bits(v), bits(flow), levels, left))
    return out


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {}])
def test_schedules(env):
    """the queue alone, tile passes to the end, the default (the switches are read once per process: a fresh child each), held
    to this process's results, which the other tests hold to the reference: identical bits of V and I across the three"""
    import re
    here = schedule_results()
    assert here[-1][4] > 0 and here[0][4] == 0
    r = run_child("from test_gpu_fwd_accum import schedule_results\nprint('RESULTS', schedule_results())\nprint('CHILD-OK')",
                  env=dict(env, PYDEM_DIST_DEBUG='1'), timeout=300)
    there = eval(r.stdout.split('RESULTS', 1)[1].splitlines()[0])
    assert [(a[0], a[1], a[2], a[4]) for a in there] == [(a[0], a[1], a[2], a[4]) for a in here]
    # what each schedule got to do: "fwd_accum: <open> open cells, <visits> tile visits finished <cells>, queue: <levels> levels, ..."
    log = {}
    for block in r.stderr.split('--- ')[1:]:
        mt = re.search(r'fwd_accum: (\d+) open cells, (\d+) tile visits finished (\d+), queue: (\d+) levels, (\d+) cells', block)
        log.setdefault(block.split()[0], []).append(tuple(int(x) for x in mt.groups()))
    assert sorted(log) == ['deep', 'fractal', 'two_loops'] and all(len(rows) == 4 for rows in log.values())
    deep_depth = deep_ramp_depth()
    for name, rows in log.items():
        for (n_open, visits, by_passes, qlevels, qcells), res in zip(rows, [a for a in there if a[0].split(' ')[0] == name]):
            print(env, name, (n_open, visits, by_passes, qlevels, qcells), res[3:])
            if env.get('PYDEM_DIST_PASSES') == '0':
                assert visits == 0 and by_passes == 0 and qcells == n_open - res[4]       # the queue alone gives the complete result
                if name == 'deep':
                    assert res[3] == deep_depth                                          # ... in the reference's levels
            elif 'PYDEM_DIST_MIN_PER_VISIT' in env:
                assert by_passes == n_open - res[4] or qlevels > 0                       # (cycles: the queue confirms that nothing is ready)
                if name == 'deep':
                    assert res[3] < deep_depth                     # a pass finishes whole chains inside a block, not one cell of each
            elif name == 'deep':
                assert visits > 0 and qlevels > 0 and qcells > 0                         # the deep ramp reaches the queue by default


# ---- 8. state
def test_state_integrity():
    """the calls write nothing but their own state: fields, graph words, pit lists and timings are bit-equal around them; the
    three other sweeps, whose planes they share (the seed plane of the reverse accumulation included), give the same bits
    before and after; a repeated call gives the same bits"""
    from pydem_amd import DEMProcessor, synth
    shape = (260, 350)
    z = synth.fractal(shape[0], shape[1], seed=11, top_shift=7, n_octaves=7)
    w, k, s = loads(shape, 4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions(); dp.run_uca(); dp.run_twi()
        up0 = dp.calc_dist_up(kind='s', stat='ave')
        racc0, dmax0 = dp.calc_rev_accum(w)
        down0 = dp.calc_dist_down(uca_threshold=300 * 900.0, kind='s', stat='ave')
        before = _snapshot(dp)
        assert len(before[0]) >= 10
        named = {f: np.array(getattr(dp, f)) for f in ('uca', 'section', 'proportion', 'edge_todo', 'mag', 'flats')}
        a = dp.calc_decay_accum(w, decay=k)
        T, D = dp.calc_trans_lim_accum(s, 3.0, edge_nan=False)
        assert np.isfinite(a).any() and np.isfinite(T).all() and (D > 0).any() and not np.array_equal(a, T, equal_nan=True)
        _same_snapshot(before, _snapshot(dp))
        for f, v in named.items():
            assert np.array(getattr(dp, f)).tobytes() == v.tobytes(), f
        assert dp.calc_dist_up(kind='s', stat='ave').tobytes() == up0.tobytes()
        T1, D1 = dp.calc_trans_lim_accum(s, 3.0, edge_nan=False)
        racc1, dmax1 = dp.calc_rev_accum(w)
        assert racc1.tobytes() == racc0.tobytes() and dmax1.tobytes() == dmax0.tobytes()
        dp.calc_trans_lim_accum(s, 3.0, edge_nan=False)
        assert dp.calc_dist_down(uca_threshold=300 * 900.0, kind='s', stat='ave').tobytes() == down0.tobytes()
        assert T1.tobytes() == T.tobytes() and D1.tobytes() == D.tobytes() and T1 is not T
        assert dp.calc_decay_accum(w, decay=k).tobytes() == a.tobytes()
        _same_snapshot(before, _snapshot(dp))


# ---- 9. memory
def test_memory():
    """the state is the sweeps' result plane and int32 plane, 12 B per cell, and four words per 32 x 32 block behind 16 counter
    words, plus 8 B per cell for the load and for each of mult, cap and inflow that a call has used: taken by the first call
    that needs it, nothing by a second call, nothing more by a later calc_dist_up"""
    from pydem_amd import DEMProcessor, _ffi, synth
    n, m = 333, 450
    z = synth.fractal(n, m, seed=23, top_shift=7, n_octaves=7)
    w, k, s = loads((n, m), 5)
    blocks = -(-n // 32) * -(-m // 32)
    state = lambda planes: (12 + 8 * planes) * n * m + 4 * (16 + 4 * blocks)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions(); dp.run_uca()
        b0 = dp._tile.device_bytes()
        first = dp.calc_decay_accum(w)                                   # the load
        b1 = dp._tile.device_bytes()
        assert 0 < b1 - b0 <= state(1), (b0, b1)
        assert dp.calc_decay_accum(w).tobytes() == first.tobytes() and dp._tile.device_bytes() == b1
        dp.calc_decay_accum(w, decay=k)                                  # + mult
        b2 = dp._tile.device_bytes()
        assert b1 < b2 <= b0 + state(2), (b0, b1, b2)
        T, D = dp.calc_trans_lim_accum(s, 3.0)                           # + cap + inflow
        b3 = dp._tile.device_bytes()
        assert b2 < b3 <= b0 + state(4), (b0, b2, b3)
        free1 = _ffi.device_memory(0)[0]
        for _ in range(3):
            T1, D1 = dp.calc_trans_lim_accum(s, 3.0)
            assert T1.tobytes() == T.tobytes() and D1.tobytes() == D.tobytes()
            dp.calc_decay_accum(w, decay=k)
        assert dp._tile.device_bytes() == b3 and _ffi.device_memory(0)[0] >= free1
        dp.calc_dist_up()
        assert dp._tile.device_bytes() == b3
        # a tile of its own whose first call uses everything at once
        dp2 = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp2.run_slopes_directions(); dp2.run_uca()
        c0 = dp2._tile.device_bytes()
        dp2._tile.fwd_accum(s, k, np.full((n, m), 3.0), True, inflow=True)
        c1 = dp2._tile.device_bytes()
        assert 0 < c1 - c0 <= state(4), (c0, c1)
        dp2._tile.fwd_accum(s, k, np.full((n, m), 3.0), True, inflow=True)
        assert dp2._tile.device_bytes() == c1


# ---- 10. errors
def test_errors():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    ones = np.ones((64, 80))
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.fwd_accum(ones)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        v = dp.calc_decay_accum(1.0, edge_nan=False)                        # runs calc_uca first
    assert np.isfinite(v).all() and (v >= 1.0).all() and dp._has('uca')
    bad = np.full((64, 80), 5.0)
    bad[63, 79] = np.nan
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp._tile.fwd_accum(ones, None, bad)
    with pytest.raises(_ffi.HipError, match='error -2'):
        _ffi.check(dp._tile.lib.pydem_fwd_accum(dp._tile._h, None, None, None, 1, None, None, None, None, None))   # no load
    with pytest.raises(ValueError):
        dp._tile.fwd_accum(np.ones((64, 79)))
    assert dp.calc_decay_accum(1.0, edge_nan=False).tobytes() == v.tobytes()  # the refused calls left the state alone
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                     # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.fwd_accum(ones)
