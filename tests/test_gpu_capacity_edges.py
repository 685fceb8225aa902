"""The device kernels at their fixed capacities: terrain from tests/capacity_terrain.py built to sit exactly at a list / window
size of the pit search (csrc/pits.hip, pits_row.inl) or the UCA sweep (csrc/uca.hip, uca_sym.inl), and one cell past it, so
the overflow hand-overs and fall-backs run; and drain_pits_max_dist=None, where the pit -> drain row spans exceed 128 and the
pairwise sums take numpy's split (pits.hip np_pairwise_sum, cond_paths.hip np_sum_dev).
Every case checks the device against the CPU oracle (pit pairs, and here the weights and patched slopes bit for bit: both sides
follow numpy's operation order without contraction) and shows it reached its target (a tier counter, a debug line or a count
taken on the host).  Schedule switches read once per process run in a subprocess, one at a time."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import capacity_terrain as CT
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (constructor, kwargs of the search).  Capacities: the lane pass's border list (LN_B = 32), the wavefront pass's
# drain list (WV_MAXD = 64), the workgroup pass's drain list (MAXD_LARGE = 2048) and its 640 x 640 window.
PIT_CASES = {
    'lane_border_32': (lambda: CT.crater(3, 32), {}),
    'lane_border_33': (lambda: CT.crater(3, 5, dent=True), {}),
    'lane_border_32_flat': (lambda: CT.crater(3, 32, cone=False), {}),
    'wave_drains_64': (lambda: CT.crater(7, 64), {}),
    'wave_drains_64_wide': (lambda: CT.crater(8, 64), {}),          # the floor of wave_drains_65: only the drain count differs
    'wave_drains_65': (lambda: CT.crater(8, 65), {}),
    'wave_drains_65_int16': (lambda: CT.crater(8, 65, dtype=np.int16), {}),
    'wave_drains_64_noise': (lambda: CT.crater(7, 64, noise=0.5, seed=3), {}),
    'wave_drains_63': (lambda: CT.crater(7, 63), {}),
    'block_drains_2048': (lambda: CT.crater(255, 2048), dict(drain_pits_max_dist=None)),
    'block_drains_2049': (lambda: CT.crater(256, 2049), dict(drain_pits_max_dist=None)),
    'reach_none_f64': (lambda: CT.channel_plateau(320), dict(drain_pits_max_dist=None)),
    'reach_none_int16': (lambda: CT.channel_plateau(330, dtype=np.int16, seed=4), dict(drain_pits_max_dist=None)),
    'reach_none_noise': (lambda: CT.channel_plateau(310, noise=0.3, seed=5), dict(drain_pits_max_dist=None)),
}


def _device_and_oracle(z, dX, dY, **opt):
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o = O.OracleDEM(z, dX=dX, dY=dY, drain_pits=True, **opt)
        o.calc_twi()
        dp = DEMProcessor(elev=z, dX=dX, dY=dY, fill_flats=False, drain_pits_path=False, drain_pits=True, **opt)
        twi = dp.calc_twi()
    return dp, o, twi


def _check_parity(dp, o, twi):
    src, dst, w = dp._tile.pit_edges()
    ref = sorted(zip(o.pit_i.tolist(), o.pit_j.tolist(), o.pit_prop.tolist()))
    got = sorted(zip(src.tolist(), dst.tolist(), w.tolist()))
    assert [r[:2] for r in ref] == [g[:2] for g in got], "pit -> drain assignments differ"
    bad = [(r, g) for r, g in zip(ref, got) if not (r[2] == g[2] or (r[2] != r[2] and g[2] != g[2]))]
    assert not bad, "%d pit weights differ (numpy summation order), first %r" % (len(bad), bad[:3])
    assert dp.timings['n_pits_undrained'] == o.n_warn
    pits = np.unique(o.pit_i)
    assert np.array_equal(dp.mag.ravel()[pits], o.mag.ravel()[pits]), "patched pit slopes differ"
    _close(dp.mag, o.mag, 'mag')
    assert np.array_equal(dp.flats, o.flats.astype(bool))
    assert np.array_equal(dp.section, o.section)
    _close(dp.uca, o.uca, 'uca')
    assert np.array_equal(dp.edge_todo, o.edge_todo)
    assert np.array_equal(dp.edge_done, o.edge_done)
    _close(twi, o.twi / 10, 'twi')


def _reach(name, info, dp, o, m):
    """the case reached its capacity: tier counters of the device, counts of the oracle"""
    tm = dp.timings
    lane_over = tm['n_pits_row'] or tm['n_pits_wave']
    cnt = np.bincount(o.pit_i, minlength=o.elev.size) if o.pit_i.size else np.zeros(o.elev.size, int)
    if name.startswith('lane_border'):
        assert info['border'] == int(name.split('_')[2]) and cnt[info['pit']] == info['drains'], (info, cnt[info['pit']])
        # 32 border cells fit the lane list; 33 go on to the next pass
        assert lane_over == (1 if info['border'] > 32 else 0), (info, tm)
    elif name.startswith('wave_drains'):
        assert cnt[info['pit']] == info['drains'] == int(name.split('_')[2]), (info, cnt[info['pit']])
        assert lane_over >= 1, tm                                        # the 17 x 17 region leaves the 16 x 16 lane window
        assert tm['n_pits_big'] == (1 if info['drains'] > 64 else 0), tm
    elif name.startswith('block_drains'):
        assert cnt[info['pit']] == info['drains'], (info, cnt[info['pit']])
        assert tm['n_pits_big'] >= 1, tm                                 # the 513-cell region needs the 640 x 640 workgroup pass
    else:
        span = CT.row_spans(o.pit_i, o.pit_j, m)
        for lo, hi in ((1, 8), (127, 129), (136, 137), (257, 1 << 30)):
            assert ((span >= lo) & (span <= hi)).any(), (lo, hi, span.max())


@pytest.mark.parametrize('name', sorted(PIT_CASES))
def test_pit_case(name):
    make, opt = PIT_CASES[name]
    z, info = make()
    dX, dY = CT.spacing(z.shape[0], seed=len(name))
    dp, o, twi = _device_and_oracle(z, dX, dY, **opt)
    _check_parity(dp, o, twi)
    _reach(name, info, dp, o, z.shape[1])


def test_reach_none_spans_feel_the_split():
    """the unbounded-reach case can tell numpy's split (n2 -= n2 % 8) from a plain halving: pairs whose dY sum differs"""
    from oracle import oracle as O
    z, _ = CT.channel_plateau(320)
    dX, dY = CT.spacing(z.shape[0], seed=len('reach_none_f64'))
    o = O.OracleDEM(z, dX=dX, dY=dY, drain_pits_max_dist=None)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    m = z.shape[1]
    differ = 0
    for a, b in zip(o.pit_i // m, o.pit_j // m):
        a, b = min(a, b), max(a, b)
        differ += np.add.reduce(dY[a:b]) != CT.np_sum_split_mutant(dY[a:b])
    assert differ >= 20, differ


def _slopes(z, dX, dY, pit, drains):
    """s of the reference (:1346-1361) for the drains of one pit, in ascending cell order"""
    m = z.shape[1]
    ip, jp = divmod(int(pit), m)
    s = []
    for d in sorted(int(x) for x in drains):
        i, j = divmod(d, m)
        a, b = min(ip, i), max(ip, i)
        dxm = dX[min(ip, dX.size - 1)] if a == b else dX[a:b].mean()
        dy = dY[a:b].sum()
        s.append(abs(float(z.flat[pit]) - float(z.flat[d])) / np.sqrt((dxm * (jp - j)) ** 2 + dy ** 2))
    return np.array(s)


def test_wave_drains_63_feel_the_drain_order():
    """the 63 tied drains of wave_drains_63: numpy's sum of their slopes in ascending cell order differs from the sum in the
    opposite order, so a wavefront pass that lists its drains the wrong way round changes the weights"""
    from oracle import oracle as O
    z, info = CT.crater(7, 63)
    dX, dY = CT.spacing(z.shape[0], seed=len('wave_drains_63'))
    o = O.OracleDEM(z, dX=dX, dY=dY)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    sel = o.pit_i == info['pit']
    s = _slopes(z, dX, dY, info['pit'], o.pit_j[sel])
    assert np.array_equal(np.sort(s / np.add.reduce(s)), np.sort(o.pit_prop[sel]))      # the restatement is the oracle's
    assert np.add.reduce(s) != np.add.reduce(s[::-1])


def test_block_pass_debug_line():
    """PYDEM_PITS_DEBUG: the 2048- and the 2049-drain crater are each the one pit that leaves the 256 x 256 pass for the
    workgroup pass; the 2048 drains fit its drain list, the 2049 are solved a second time with room for a full window"""
    script = ("import sys, warnings; sys.path[:0] = [%r, %r]; warnings.simplefilter('ignore')\n"
              "import test_gpu_capacity_edges as T\n"
              "for a, nd in ((255, 2048), (256, 2049)):\n"
              "    z, info = T.CT.crater(a, nd)\n"
              "    dp, o, twi = T._device_and_oracle(z, *T.CT.spacing(z.shape[0]), drain_pits_max_dist=None)\n"
              "    T._check_parity(dp, o, twi)\n"
              "    print('CAP-OK', nd, file=sys.stderr, flush=True)\n") % (ROOT, os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, PYDEM_PITS_DEBUG='1'), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and 'CAP-OK 2049' in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    first, second = r.stderr.split('CAP-OK 2048')
    for part, again in ((first, 0), (second, 1)):
        left = re.findall(r'(\d+) left the 256x256 / 2048-cell pass', part)
        assert left and int(left[-1]) == 1, part[-2000:]
        solved = re.findall(r'(\d+) pits with more than 2048 drains solved again', part)
        assert solved and int(solved[-1]) == again, part[-2000:]


# --- the UCA sweep -------------------------------------------------------------------------------------------------------

def _sweep_case(kind):
    if kind == 'egg_crate':
        return CT.egg_crate(256, 288)
    if kind == 'egg_crate_noise':
        return CT.egg_crate(256, 256, noise=0.4, seed=2)
    if kind == 'funnel':
        return CT.funnel(512)
    return CT.funnel(512, holes=12, seed=1)


@pytest.mark.parametrize('kind', ['egg_crate', 'egg_crate_noise', 'funnel', 'funnel_pit_inlets'])
def test_sweep_case(kind):
    """egg crate: > 256 cells of a 32 x 32 tile have no in-edge, so the first pass overflows the tile's ready ring
    (TILE_RING = 256); funnel: the halo of the tile under the bowl's centre delivers 132 inlets (SYM_MAXIN = 64), or 120 plus
    pit sources from the sinks around it"""
    z = _sweep_case(kind)
    dp, o, twi = _device_and_oracle(z, 30.0, 30.0)
    _check_parity(dp, o, twi)
    if kind.startswith('egg'):
        assert CT.max_sources_per_tile(CT.in_degree(o.A, z.size), z.shape) > 256
    else:
        halo, pit_src = CT.tile_inlets(o.A, z.shape, 8, 8)
        assert halo + pit_src > 64, (halo, pit_src)
        if kind == 'funnel_pit_inlets':
            assert pit_src > 0


def test_two_level_solve_falls_back_on_the_funnel():
    """PYDEM_SWEEP_SYM=100000000 (the symbolic pass right after two full passes) on the funnel: the tiles still listed then
    take the numeric visits instead of the two-level solve, and the answer stays the oracle's.  (The debug line counts the
    fall-backs but not which limit caused them -- inlets, open cells or the pool -- so this does not single out SYM_MAXIN.)"""
    script = ("import sys, warnings; sys.path[:0] = [%r, %r]; warnings.simplefilter('ignore')\n"
              "import test_gpu_capacity_edges as T\n"
              "dp, o, twi = T._device_and_oracle(T._sweep_case('funnel'), 30.0, 30.0)\n"
              "T._check_parity(dp, o, twi)\nprint('CAP-OK')\n") % (ROOT, os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, PYDEM_SWEEP_SYM='100000000', PYDEM_SWEEP_DEBUG='1'),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and 'CAP-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    fb = re.findall(r'symbolic tiles \((\d+) fell back to numeric visits\)', r.stderr)
    assert fb and int(fb[-1]) >= 1, r.stderr[-2000:]


# --- conditioning: calc_pit_drain_paths with drain_pits_max_dist=None --------------------------------------------------

@pytest.mark.parametrize('length,dtype', [(300, np.float64), (290, np.int16)])
def test_pit_paths_unbounded_reach_match_host_twin(length, dtype):
    """a strict minimum at the head of a 300-row channel: its outlet search walks the whole channel (300 iterations, a path of
    300 cells); device against the host twin, bit for bit.  (The outlet reaches sum dY over 300 rows here, but the outlet
    choice does not hang on their last bit: test_pit_paths_outlet_choice_turns_on_the_split is the case that does.)"""
    import conditioning_numpy as CN
    from pydem_amd import DEMProcessor
    z, info = CT.channel_plateau(length, pit_at_head=True, dtype=dtype)
    dX, dY = CT.spacing(z.shape[0], seed=length)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want, bad, used = CN.pit_drain_paths(z.copy(), dX, dY, drain_pits_max_dist=None)
        dp = DEMProcessor(elev=z.copy(), dX=dX, dY=dY, fill_flats=False, drain_pits_max_dist=None)
        res = dp._pit_paths_on_device()
        assert res is not None, "the device paths fell back to the host loop"
        got = np.asarray(dp.elev)
    rows = np.nonzero((want != z).any(axis=1))[0]
    assert rows.size and rows.max() - rows.min() > 128, rows
    assert got.dtype == want.dtype and np.array_equal(got, want), "paths differ on %d cells" % int((got != want).sum())
    assert res[0] == bad and res[1] == used, (res, bad, used)


@pytest.mark.parametrize('seed', [25, 27, 32])
def test_pit_paths_outlet_choice_turns_on_the_split(seed):
    """two outlets of one elevation 150 rows above and below a pit, reached in the same iteration: the path goes to the one
    whose dY sum (cond_paths.hip np_sum_dev) is smaller, the upper one on a tie.  The two sums are within an ulp or two of each
    other and their order flips when numpy's split (n2 -= n2 % 8) is lost -- shown on the host twin -- so the device must
    sum like numpy to carve the same path.  (seed 25: a tie, the upper outlet; 27: the lower one; 32: the upper, by an ulp)"""
    import conditioning_numpy as CN
    from pydem_amd import DEMProcessor
    z, dX, dY, info = CT.twin_outlets(seed=seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want, bad, used = CN.pit_drain_paths(z.copy(), dX, dY, drain_pits_max_dist=None)
        wrong, _, _ = CN.pit_drain_paths(z.copy(), dX, dY.view(CT.SplitMutantSum), drain_pits_max_dist=None)
        dp = DEMProcessor(elev=z.copy(), dX=dX, dY=dY, fill_flats=False, drain_pits_max_dist=None)
        res = dp._pit_paths_on_device()
        assert res is not None, "the device paths fell back to the host loop"
        got = np.asarray(dp.elev)
    up = bool((want[:info['pit'] // z.shape[1]] != z[:info['pit'] // z.shape[1]]).any())
    assert up == (info['rise_up'] <= info['rise_down']) and bad == 0, (up, info, bad)
    assert not np.array_equal(wrong, want), "the case does not tell numpy's split from a plain halving"
    assert np.array_equal(got, want), "paths differ on %d cells" % int((got != want).sum())
    assert res[0] == bad and res[1] == used, (res, bad, used)


# --- the same cases under the other schedules (read once per process: a subprocess each, one at a time) -------------------

@pytest.mark.parametrize('env', [{'PYDEM_PITS_ROW': '0'}, {'PYDEM_PITS_ROW': '2'}, {'PYDEM_PITS_HANDOVER': '0'}])
def test_pit_cases_under_schedule(env):
    # (the node id picks test_pit_case: a keyword alone would match these schedule tests too, and the child would start
    # children of its own; -k then only drops the two large craters)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__) + '::test_pit_case', '-q', '-x', '-p',
                        'no:cacheprovider', '-k', 'not 2048 and not 2049'], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and ' passed' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize('sym', ['0', '100000000'])
def test_sweep_cases_under_schedule(sym):
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__) + '::test_sweep_case', '-q', '-x', '-p',
                        'no:cacheprovider'], env=dict(os.environ, PYDEM_SWEEP_SYM=sym), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and ' passed' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
