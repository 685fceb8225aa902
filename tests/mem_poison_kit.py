"""The scenarios of tests/test_gpu_mem_poison.py: every device path that takes its memory from csrc/devmem.hip (the plane cache,
dev_malloc, the conditioning arena), each at the smallest shapes its own GPU test uses, run once per child process under one
setting of PYDEM_MEM_POISON.  A plain module: no tests, no marks; the device is touched by the scenarios only.

A scenario is (name, run, check): run() builds its inputs, runs ONE device path and returns ({output name: ndarray}, context);
check(outputs, context) holds the outputs to the host reference the project already has for that path, with the comparator and the
tolerance of the path's own GPU test, imported from that test.  main() runs them all and prints one JSON object: per scenario the
sha256 digests of its outputs (flowgraph_kit.bits for any dtype), with `anchor` the verdict of check(), and what
_ffi.poison_stats() said around each scenario."""
import gc
import hashlib
import json
import os
import time
import traceback
import warnings

import numpy as np

MODES = {'unset': None, '0x00': '0', '0xFF': '255', '0x7F': '127'}
RESULT_TAG = 'MEM-POISON-RESULT '
EXTRA = {}                  # what a scenario measured besides its outputs (main() ships it)


def digest(a):
    """sha256 of the array's own bytes, dtype and shape (flowgraph_kit.bits ships float64 planes; the tables here are integers)"""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(('%s %r ' % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def flatten(out):
    """{name: ndarray} with structured arrays split into their columns (their padding bytes mean nothing)"""
    flat = {}
    for name, a in out.items():
        a = np.asarray(a)
        if a.dtype.names:
            for col in a.dtype.names:
                flat['%s.%s' % (name, col)] = a[col]
        else:
            flat[name] = a
    return flat


def _arr(a):
    return np.array(np.asarray(a))


# ---- 1. the pipeline from raw input with the reference's defaults (test_gpu_parity.test_full_pipeline_with_conditioning)
PIPELINE_GOLDENS = ('g7_nan_lakes', 'g7_int16_terraces', 'g5_f32_defaults', 'g4_fractal_pits')


def run_pipeline(name):
    from conftest import load_golden
    from pydem_amd import DEMProcessor
    g = load_golden(name)
    dp = DEMProcessor(elev=g['in_elev'], dX=g['in_dX'], dY=g['in_dY'], dX2=g['in_dX2'], dY2=g['in_dY2'], **g['kwargs'])
    twi = dp.calc_twi()
    out = dict(elev=np.asarray(dp.elev, float), mag=_arr(dp.mag), direction=_arr(dp.direction), flats=_arr(dp.flats),
               section=_arr(dp.section), uca=_arr(dp.uca), edge_todo=_arr(dp.edge_todo), edge_done=_arr(dp.edge_done),
               twi=_arr(twi), twi_attr=_arr(dp.twi))
    return out, g


def check_pipeline(out, g):
    from test_gpu_parity import _close
    assert np.array_equal(out['elev'], g['elev_final'].astype(float), equal_nan=True)
    _close(out['mag'], g['mag_final'], 'mag')
    _close(out['direction'], g['direction'], 'direction')
    assert np.array_equal(out['flats'], g['flats_final'])
    assert np.array_equal(out['section'], g['section'])
    _close(out['uca'], g['uca'], 'uca')
    assert np.array_equal(out['edge_todo'], g['edge_todo'])
    assert np.array_equal(out['edge_done'], g['edge_done'])
    _close(out['twi'], g['twi_ret'], 'twi')
    _close(out['twi_attr'], g['twi_attr'], 'twi attr')


# ---- 2. one edge-update round (test_gpu_edge_update.test_hip_edge_update_vs_reference_golden), the operator build both ways
EDGE_GOLDENS = ('g6_edge_update_pits', 'g6_edge_update_quant')


def run_edge_round(name):
    from conftest import load_golden
    from pydem_amd import DEMProcessor
    from test_gpu_edge_update import _strips
    g = load_golden(name)
    kw = g['kwargs']
    out = {}
    saved = os.environ.pop('PYDEM_COND_BUILD', None)
    try:
        for how in ('device', 'host'):
            if how == 'host':
                os.environ['PYDEM_COND_BUILD'] = 'host'         # (as test_gpu_edge_forms.FORMS['condensed-host'] sets it)
            dp = DEMProcessor(elev=g['in_elev'], dX=g['in_dX'], dY=g['in_dY'], dX2=g['in_dX2'], dY2=g['in_dY2'], mag=g['in_mag'],
                              direction=g['in_direction'], fill_flats=False, drain_pits_path=False, drain_pits=kw.get('drain_pits', True))
            dp.find_flats()
            strips = [_strips(g, 'data'), _strips(g, 'done'), _strips(g, 'todo')]
            uca = dp.calc_uca(uca_init=g['uca_init'], edge_init_data=strips)
            out.update({how + '.uca': _arr(uca), how + '.edge_todo': _arr(dp.edge_todo), how + '.edge_done': _arr(dp.edge_done)})
            # ... and the same strips once more as an incremental round on the resident plane, which builds the condensed operator
            # the way PYDEM_COND_BUILD says, then the flush
            dp.run_uca(edge_init_data=strips, uca_resident=True, incremental=True)
            dp.flush_edge_rounds()
            out.update({how + '.inc.uca': _arr(dp.uca), how + '.inc.edge_todo': _arr(dp.edge_todo), how + '.inc.edge_done': _arr(dp.edge_done)})
    finally:
        os.environ.pop('PYDEM_COND_BUILD', None)
        if saved is not None:
            os.environ['PYDEM_COND_BUILD'] = saved
    return out, g


def check_edge_round(out, g):
    from test_gpu_parity import _close
    for how in ('device', 'host'):
        _close(out[how + '.uca'], g['uca'], 'uca after edge round (%s)' % how)
        assert np.array_equal(out[how + '.edge_todo'], g['edge_todo'])
        assert np.array_equal(out[how + '.edge_done'], g['edge_done'])
    # (the incremental round has no golden: its outputs are held across the modes, and across the two builds -- whose edge
    # weights agree to 1e-12 relative, not to the bit -- by the bars of test_gpu_edge_forms after a flush)
    _close(out['device.inc.uca'], out['host.inc.uca'], 'uca after the flush, device build against host build')
    for key in ('inc.edge_todo', 'inc.edge_done'):
        assert np.array_equal(out['device.' + key], out['host.' + key]), key


# ---- 3. the flow-graph analyses, on one handle, in one order, and the first sweep once more at the end
FLOW_SHAPE = (130, 67)
FLOW_CELLS = 20             # stream / target threshold, in cells of 900 m^2


def run_flowgraph(kind):
    import flowgraph_kit as K
    if kind == 'fractal':
        o, dp = K.fractal_pair(FLOW_SHAPE, 14)
    else:
        _, o, dp, _ = K.nan_speck_pair(FLOW_SHAPE, 6, [(0, 5), (FLOW_SHAPE[0] - 1, 30), (60, 0)])
    z = np.asarray(o.elev, np.float64)
    thr = FLOW_CELLS * 900.0
    rng = np.random.default_rng(8)
    w = K.random_weights(FLOW_SHAPE, 3)
    decay, supply = rng.uniform(0.5, 1.0, FLOW_SHAPE), rng.uniform(0.0, 2.0, FLOW_SHAPE)
    load = rng.normal(0.0, 3.0, FLOW_SHAPE)
    out = {'uca': _arr(dp.uca), 'mag': _arr(dp.mag)}
    out['weighted_uca'] = _arr(dp.calc_weighted_uca(w))
    out['dist_down_h_ave'] = _arr(dp.calc_dist_down(uca_threshold=thr, kind='h', stat='ave'))
    out['dist_down_v_max'] = _arr(dp.calc_dist_down(uca_threshold=thr, kind='v', stat='max'))
    out['dist_up'] = _arr(dp.calc_dist_up())
    racc, dmax = dp.calc_rev_accum(w)
    out['rev_accum_sum'], out['rev_accum_max'] = _arr(racc), _arr(dmax)
    out['decay_accum'] = _arr(dp.calc_decay_accum(w, decay=decay))
    T, D = dp.calc_trans_lim_accum(supply, 3.0)
    out['trans_lim_transport'], out['trans_lim_deposition'] = _arr(T), _arr(D)
    net = dp.calc_stream_network(uca_threshold=thr)
    for name in ('receiver', 'order', 'link', 'basin', 'links'):
        out['net_' + name] = _arr(getattr(net, name))
    out['tree_accum'] = _arr(dp.calc_tree_accum(load, op='sum', uca_threshold=thr))
    out['reach_table'] = _arr(dp.calc_reach_attributes(uca_threshold=thr, values=out['mag']))
    out['dist_down_again'] = _arr(dp.calc_dist_down(uca_threshold=thr, kind='h', stat='ave'))
    return out, dict(o=o, dp=dp, z=z, thr=thr, w=w, decay=decay, supply=supply, load=load)


def check_flowgraph(out, c):
    import flowgraph_kit as K
    import test_gpu_dist_down as DD
    import test_gpu_dist_up as DU
    import test_gpu_fwd_accum as FA
    import test_gpu_rev_accum as RA
    import test_gpu_stream_network as SN
    import test_gpu_weighted_uca as WU
    from pydem_amd import streamnet
    from test_stream_network_ref import stream_network_ref
    from test_tree_accum_ref import reach_table_ref, tree_accum_ref
    o, dp, z, thr, w = c['o'], c['dp'], c['z'], c['thr'], c['w']
    K.assert_bound(out['weighted_uca'], WU.weighted_ref(o, w), WU.weighted_ref(o, np.abs(w)), 'weighted uca', WU.BOUND)
    with np.errstate(invalid='ignore'):
        target = out['uca'] >= thr
    DD.compare(out['dist_down_h_ave'], o, target, 'h', 'ave', 'dist_down h/ave')
    DD.compare(out['dist_down_v_max'], o, target, 'v', 'max', 'dist_down v/max')
    DU.compare(out['dist_up'], o, 'h', 'max', True, 'dist_up h/max')
    RA.compare(out['rev_accum_sum'], o, 0, 'rev_accum sum', seed=w)
    RA.compare(out['rev_accum_max'], o, 1, 'rev_accum max', seed=w)
    FA.compare(out['decay_accum'], None, o, w, c['decay'], None, True, 'decay_accum')
    (V, I, _, _), (Va, _, _, _) = FA.reference(o, c['supply'], None, 3.0, True)
    K.assert_bound(out['trans_lim_transport'], V, Va, 'trans_lim T', FA.BOUND)
    with np.errstate(invalid='ignore'):
        K.assert_bound(out['trans_lim_deposition'], (c['supply'] + I) - V, Va, 'trans_lim D', FA.BOUND)
    edges = SN.device_edges(dp, z)
    S = SN.stream_set(dp, thr)
    ref = stream_network_ref(edges, FLOW_SHAPE, z, S)
    want = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)
    for name in SN.PLANES:
        assert np.array_equal(out['net_' + name], getattr(want, name)), name
    assert np.array_equal(out['net_links'], want.links)
    tree, _ = tree_accum_ref(edges, FLOW_SHAPE, z, c['load'], 'sum', S, True, net=ref)
    assert out['tree_accum'].tobytes() == tree.tobytes()
    table, _ = reach_table_ref(edges, FLOW_SHAPE, z, S, dp.dX2, dp.dY2, out['mag'], True)
    for col in out['reach_table'].dtype.names:
        assert out['reach_table'][col].tobytes() == table[col].tobytes(), col
    assert out['dist_down_again'].tobytes() == out['dist_down_h_ave'].tobytes()


# ---- 4. fill and depressions, both schedules
def _fill_fields():
    import fill_fields as F
    return {'bowl_nan_hole': F.bowl_nan_hole(), 'nested': F.nested(), 'fractal70x45_nan': F.fractal(70, 45, nan_rect=True)}


def _depression_fields():
    import depression_fields as D
    return {'two_levels': D.two_levels(), 'lake_nan_hole': D.lake_nan_hole(), 'varying_spacing': D.varying_spacing()}


LIMIT_DEPTH = 20.0          # (test_gpu_depressions.test_limited_fill_on_the_device on 'limits')


def run_fill_and_depressions():
    import depression_fields as D
    import test_gpu_depressions as GD
    import test_gpu_fill_depressions as FD
    from pydem_amd import DEMProcessor
    out = {}
    saved = {k: os.environ.pop(k, None) for k in ('PYDEM_FILL_LOCAL', 'PYDEM_DEPR_LOCAL')}
    try:
        for local in ('1', '0'):
            os.environ['PYDEM_FILL_LOCAL'] = os.environ['PYDEM_DEPR_LOCAL'] = local
            for name, z in _fill_fields().items():
                for eps in (0.0, None):
                    _, W, depth, st = FD.device_fill(z, eps)
                    key = 'local%s.fill.%s.%s' % (local, name, 'auto' if eps is None else 'eps0')
                    out[key + '.W'], out[key + '.depth'] = _arr(W), _arr(depth)
                    out[key + '.counts'] = np.array([st['epsilon'], st['n_raised'], st['max_depth']], np.float64)
            for name, z in _depression_fields().items():
                _, res = GD.device(name, z)
                key = 'local%s.depr.%s' % (local, name)
                out[key + '.label'], out[key + '.table'] = _arr(res['label']), _arr(res['table'])
            dp = DEMProcessor(elev=D.limits(), dX=30.0, dY=30.0)
            out['local%s.limited.W' % local] = _arr(dp.calc_fill_depressions_limited(max_depth=LIMIT_DEPTH))
            out['local%s.limited.kept_sinks' % local] = _arr(dp.kept_sinks)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out, None


def check_fill_and_depressions(out, _):
    import depression_fields as D
    import test_gpu_depressions as GD
    import test_gpu_fill_depressions as FD
    from depression_checks import same
    from pydem_amd import conditioning
    for local in ('1', '0'):
        for name, z in _fill_fields().items():
            for eps in (0.0, None):
                rW, rdepth, reps = FD.ref('poison.' + name, z, eps)
                key = 'local%s.fill.%s.%s' % (local, name, 'auto' if eps is None else 'eps0')
                assert out[key + '.W'].tobytes() == rW.tobytes() and out[key + '.depth'].tobytes() == rdepth.tobytes(), key
                with np.errstate(invalid='ignore'):
                    up = rdepth > 0
                assert out[key + '.counts'].tolist() == [reps, float(up.sum()), float(rdepth[up].max()) if up.any() else 0.0], key
        for name, z in _depression_fields().items():
            key = 'local%s.depr.%s' % (local, name)
            same({'label': out[key + '.label'], 'table': out[key + '.table']}, GD.ref(name, z))
        z = D.limits()
        want = conditioning.fill_depressions_limited(z, max_depth=LIMIT_DEPTH, dX2dY2=D.row_area('limits', z.shape[0]))
        assert out['local%s.limited.W' % local].tobytes() == want[0].tobytes()
        assert np.array_equal(out['local%s.limited.kept_sinks' % local], want[3]) and len(want[3]) >= 1


# ---- 5. a seam session on one tile (test_gpu_depressions_mosaic.test_label_and_inventory_against_the_host_twin, relaxed twice)
SEAM_SHAPES = ((70, 45), (3, 40))


def _seam_inputs(shape):
    import test_gpu_depressions_mosaic as DM
    n, m = shape
    z = DM.surface(shape)
    seam = {s: np.ones(m if s in ('top', 'bottom') else n, bool) for s in DM.SIDES}
    line = {'top': z[0], 'bottom': z[-1], 'left': z[:, 0], 'right': z[:, -1]}
    rng = np.random.RandomState(4)
    above = {s: rng.uniform(0.0, 3.0, line[s].size) for s in DM.SIDES}
    lower = {s: above[s] * rng.uniform(0.0, 1.0, line[s].size) for s in DM.SIDES}       # (caps may only fall)
    caps = [{s: np.nan_to_num(np.array(line[s]), nan=np.inf) + d[s] for s in DM.SIDES} for d in (above, lower)]
    return z, seam, caps, [(n // 2, m // 2), (1, 1)]


def _seam_inventory_inputs(shape, z, k_local, dmax):
    import test_gpu_depressions_mosaic as DM
    from pydem_amd import conditioning
    n, m = shape
    lut, T, owner, halo_ids, row_area = DM.inventory_inputs(shape, k_local, 0)
    rng = np.random.RandomState(10)
    halo_W = np.concatenate([z[0, [0] + list(range(m)) + [m - 1]], z[-1, [0] + list(range(m)) + [m - 1]], z[:, 0], z[:, -1]])
    halo_W = np.where(rng.uniform(size=halo_W.size) < 0.7, np.nan_to_num(halo_W, nan=0.0), rng.uniform(0.0, 100.0, halo_W.size))
    sh_a, _ = conditioning.fixed_point(n * m, row_area.max())
    sh_v, _ = conditioning.fixed_point(n * m, dmax * row_area.max())
    kept = np.concatenate(([0], rng.randint(0, 5, k_local))).astype(np.int32)
    return (lut, T, owner, halo_ids, halo_W, row_area, sh_a, sh_v), kept


def run_seam_session(shape):
    import test_gpu_depressions_mosaic as DM
    n, m = shape
    z, seam, caps, outlets = _seam_inputs(shape)
    dp = DM.device(z)
    out = {'amax': np.float64(dp.fill_seam_begin(seam, outlets))}
    lowered = [dp.fill_seam_relax(0.0, c)['n_lowered'] for c in caps]
    out['n_lowered'] = np.array(lowered, np.int64)
    out['W'] = np.array(dp.fill_seam_lines([(0, r) for r in range(n)]))
    got = dp.fill_seam_label()
    out['roots'], out['levels'], out['max_depth'] = _arr(got['roots']), _arr(got['levels']), np.float64(got['max_depth'])
    out['ids'] = np.array(dp.fill_seam_id_lines([(0, r) for r in range(n)]))
    inv, kept = _seam_inventory_inputs(shape, z, out['roots'].size, float(out['max_depth']))
    out['table'] = _arr(dp.fill_seam_inventory(*inv)['table'])
    out['label'] = _arr(dp.fill_seam_labels(kept)['label'])
    commit = bool(np.isfinite(out['W'][np.isfinite(z)]).all())
    dp.fill_seam_end(commit)
    out['elev_after'] = np.asarray(dp.elev, np.float64).copy()
    return out, commit


def check_seam_session(shape, out, commit):
    import depression_mosaic_kit as D
    from pydem_amd import conditioning
    n, m = shape
    z, seam, caps, outlets = _seam_inputs(shape)
    twin = conditioning.SeamFill(z, D.outlets_mask(z.shape, outlets), seam)
    assert float(out['amax']) == twin.amax
    assert out['n_lowered'].tolist() == [twin.relax(0.0, c) for c in caps]
    assert out['W'].tobytes() == twin.W.tobytes()
    roots, levels, dmax = twin.label()
    assert np.array_equal(out['roots'], roots) and np.array_equal(out['levels'], levels) and float(out['max_depth']) == dmax
    assert roots.size >= 1 and np.array_equal(out['ids'], twin.ids)
    inv, kept = _seam_inventory_inputs(shape, z, roots.size, dmax)
    assert np.array_equal(out['table'], twin.inventory(*inv))
    assert np.array_equal(out['label'], twin.labels(kept))
    assert commit == (not np.isinf(twin.W).any())
    want = twin.end(True)[0] if commit else z
    assert out['elev_after'].tobytes() == np.ascontiguousarray(want, np.float64).tobytes()


# ---- 6. mosaics on one GPU
MOSAIC_FIELD = 'designed_nan'
MOSAIC_CUTS = ((2, 2, 1), (3, 3, 2))


def run_fill_mosaic(cut):
    import depression_mosaic_kit as D
    import seam_fill_kit as K
    from pydem_amd import DEMProcessor
    pm = K.manager(D.field(MOSAIC_FIELD), *cut, processor_cls=DEMProcessor, devices=[0])
    lat = pm.fill_lattice()
    pm.process_fill_depressions(None)
    out = {'tile%d.elev' % i: np.asarray(t.elev, np.float64).copy() for i, t in enumerate(pm.tiles)}
    out['epsilon'] = np.float64(pm.fill_depressions_epsilon_used)
    return out, (pm, lat)


def check_fill_mosaic(cut, out, c):
    import seam_fill_kit as K
    pm, lat = c
    W = K.whole_fill(('poison', MOSAIC_FIELD, cut), K.stitched(pm, lat), None)
    K.assert_tiles_equal_whole(pm, lat, W)
    for i in range(pm.n_inputs):
        assert out['tile%d.elev' % i].tobytes() == np.asarray(pm.tiles[i].elev, np.float64).tobytes()


def run_depressions_mosaic(cut):
    import depression_mosaic_kit as D
    from pydem_amd import DEMProcessor
    pm = D.manager(D.field(MOSAIC_FIELD), *cut, spacing=True, processor_cls=DEMProcessor, devices=[0])
    lat = pm.fill_lattice()
    pm.process_elevation()
    res = pm.process_depressions()
    out = {'table': _arr(res['table'])}
    out.update({'tile%d.label' % i: _arr(lab) for i, lab in enumerate(res['labels'])})
    return out, (pm, lat, res)


def check_depressions_mosaic(cut, out, c):
    import depression_mosaic_kit as D
    pm, lat, res = c
    D.assert_equals_whole(pm, lat, res, D.whole(('poison', MOSAIC_FIELD, cut), pm, lat))


PM_GOLDEN = 'pm_cone32_3x3_ov2'
PM_KEYS = ('uca_total', 'edge_todo', 'edge_done', 'twi')


def _run_pm(queue, sub):
    import tempfile
    from conftest import load_golden
    from test_process_manager_cpu import run_pm
    saved = os.environ.pop('PYDEM_EDGE_QUEUE', None)
    if queue is not None:
        os.environ['PYDEM_EDGE_QUEUE'] = queue
    try:
        with tempfile.TemporaryDirectory() as d:
            pm, compact, _ = run_pm(load_golden(PM_GOLDEN), os.path.join(d, sub), n_workers=8, tiles_in_flight=2)
            out = {'tile%d.%s' % (i, key): _arr(pm.tile_result(i, key)) for i in range(pm.n_inputs) for key in PM_KEYS}
            out.update({'compact.' + key: _arr(v) for key, v in compact.items()})
            counts = dict(waves=pm.edge_waves, rounds=pm.edge_rounds, tiebreaks=pm.edge_tiebreaks, batches=pm.edge_queued_batches)
    finally:
        os.environ.pop('PYDEM_EDGE_QUEUE', None)
        if saved is not None:
            os.environ['PYDEM_EDGE_QUEUE'] = saved
    return out, counts


def run_pm_queued_waves():
    """process_twi in pool mode with the waves chosen and queued on the device (the default): the board, its schedule and scalar
    blocks, the staging buffer and the captured wave"""
    out, counts = _run_pm(None, 'queued')
    out['counts'] = np.array([counts['waves'], counts['rounds'], counts['tiebreaks']], np.int64)
    return out, counts


def check_pm_queued_waves(out, counts):
    """test_gpu_process_manager.test_queued_waves_equal_host_driven_waves: the host-driven wave loop, bit for bit"""
    assert counts['batches'] > 0
    host, hcounts = _run_pm('0', 'host')
    assert hcounts['batches'] == 0
    assert (counts['waves'], counts['rounds'], counts['tiebreaks']) == (hcounts['waves'], hcounts['rounds'], hcounts['tiebreaks'])
    for key in host:
        assert np.array_equal(out[key], host[key], equal_nan=True), key


# ---- 7. tile memory: the A-then-B regrow of test_gpu_tile_memory
def run_tile_memory():
    import test_gpu_tile_memory as TM
    from pydem_amd import _ffi
    a, b = TM.fields()
    before = _ffi.poison_stats()
    grown = _ffi.Tile(TM.N, TM.N)
    TM.run(_ffi, grown, a)
    _, uca_grown, bytes_grown = TM.run(_ffi, grown, b)
    after = _ffi.poison_stats()
    EXTRA['tile_memory'] = dict(poisoned_bytes=after[1] - before[1], poisoned_blocks=after[0] - before[0], device_bytes=int(bytes_grown))
    fresh = _ffi.Tile(TM.N, TM.N)
    _, uca_fresh, bytes_fresh = TM.run(_ffi, fresh, b)
    grown.close(); fresh.close()
    return dict(uca_grown=uca_grown, uca_fresh=uca_fresh, device_bytes=np.array([bytes_grown, bytes_fresh], np.int64)), None


def check_tile_memory(out, _):
    assert out['uca_grown'].tobytes() == out['uca_fresh'].tobytes()
    assert out['device_bytes'][0] == out['device_bytes'][1]


# ---- 8. the free-list hit: planes of 1 MiB and more come back from the tile before
BIG_SHAPE = (1024, 1040)    # 1 064 960 cells: byte planes 1.02 MiB, int32 planes 4.1 MiB, fp64 planes 8.1 MiB
BIG_CELLS = 500


def _big_tile(seed):
    from pydem_amd import DEMProcessor, synth
    z = synth.fractal(BIG_SHAPE[0], BIG_SHAPE[1], seed=seed)
    thr = BIG_CELLS * 900.0
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=True, drain_pits_path=True, drain_pits=True)
    out = {'twi': _arr(dp.calc_twi())}
    for k in ('mag', 'direction', 'uca', 'edge_todo', 'edge_done', 'flats'):
        out[k] = _arr(getattr(dp, k))
    out['dist_down'] = _arr(dp.calc_dist_down(uca_threshold=thr))
    net = dp.calc_stream_network(uca_threshold=thr)
    for name in ('receiver', 'order', 'link', 'basin', 'links'):
        out['net_' + name] = _arr(getattr(net, name))
    W, depth = dp.calc_fill_depressions(0.0, return_depth=True)
    out['fill_W'], out['fill_depth'] = _arr(W), _arr(depth)
    res = dp.calc_depressions()
    out['depr_label'], out['depr_table'] = _arr(res['label']), _arr(res['table'])
    del dp, net, res
    gc.collect()                                    # the tile is destroyed: its planes go on the free lists
    return out


def run_free_list_hit():
    _big_tile(11)                                   # leaves its planes, full of another tile's values (or of the poison byte)
    return _big_tile(12), None


def check_free_list_hit(out, _):
    """device-only: the same run on memory mapped anew (the Python references take too long at a million cells)"""
    from pydem_amd import _ffi
    _ffi.release_scratch()
    fresh = flatten(_big_tile(12))
    for key, a in flatten(out).items():
        assert digest(a) == digest(fresh[key]), key


def _scenarios():
    from functools import partial as P
    s = []
    for name in PIPELINE_GOLDENS:
        s.append(('pipeline.' + name, P(run_pipeline, name), check_pipeline))
    for name in EDGE_GOLDENS:
        s.append(('edge_round.' + name, P(run_edge_round, name), check_edge_round))
    for kind in ('fractal', 'nan_specks'):
        s.append(('flowgraph.' + kind, P(run_flowgraph, kind), check_flowgraph))
    s.append(('fill_and_depressions', run_fill_and_depressions, check_fill_and_depressions))
    for shape in SEAM_SHAPES:
        s.append(('seam_session.%dx%d' % shape, P(run_seam_session, shape), P(check_seam_session, shape)))
    for cut in MOSAIC_CUTS:
        s.append(('fill_mosaic.%dx%d_ov%d' % cut, P(run_fill_mosaic, cut), P(check_fill_mosaic, cut)))
        s.append(('depressions_mosaic.%dx%d_ov%d' % cut, P(run_depressions_mosaic, cut), P(check_depressions_mosaic, cut)))
    s.append(('pm_queued_waves', run_pm_queued_waves, check_pm_queued_waves))
    s.append(('tile_memory', run_tile_memory, check_tile_memory))
    s.append(('free_list_hit', run_free_list_hit, check_free_list_hit))
    return s


SCENARIOS = _scenarios()
NAMES = [name for name, _, _ in SCENARIOS]


def main(anchor=False):
    """Run every scenario in this process and print the result line.  The first scenario that raises ends the run (whatever
    it left on the device, nothing more is started there); those behind it are reported as not run."""
    from pydem_amd import _ffi
    result = dict(mode=os.environ.get('PYDEM_MEM_POISON'), scenarios={}, stats_start=list(_ffi.poison_stats()))
    t_all = time.time()
    failed = None
    for name, run, check in SCENARIOS:
        if failed:
            result['scenarios'][name] = dict(error='not run: %s failed before it' % failed)
            continue
        rec = dict(stats_before=list(_ffi.poison_stats()))
        t0 = time.time()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                out, ctx = run()
                rec['digests'] = {k: digest(v) for k, v in flatten(out).items()}
                rec['stats_after'] = list(_ffi.poison_stats())
                rec['run_s'] = round(time.time() - t0, 3)
                if anchor:
                    try:
                        check(out, ctx)
                        rec['anchor'] = None
                    except AssertionError:
                        rec['anchor'] = traceback.format_exc()[-2000:]
                    rec['check_s'] = round(time.time() - t0 - rec['run_s'], 3)
        except Exception:
            rec['error'] = traceback.format_exc()[-2000:]
            failed = name
        result['scenarios'][name] = rec
        gc.collect()
    result['extra'] = EXTRA
    result['stats_end'] = list(_ffi.poison_stats())
    result['wall_s'] = round(time.time() - t_all, 2)
    print(RESULT_TAG + json.dumps(result))
    print('CHILD-OK')
