"""The four sweep engines of fill_flats (csrc/cond_device.hip, stage_fill_flats) and the hand-overs between them, on the
designed flats of tests/flat_fields.py.  The reference stops each distance of a flat in the sweep in which its last cell
gets a first value, and on a zigzag lake one more sweep changes the distances (tests/test_flat_fields.py pins both), so a
region that an engine stops a sweep late -- a missed repeat of a pass, a stop booked at the wrong sweep of a pass, a pass
boundary off by one -- gives a different surface here, which ordinary terrain never shows.

The thresholds are read once per process: one child per setting (tests/_flat_engines_worker.py) runs every field as
float64 and as int16, with maximum_pit_area 0 and the default, and dumps the surfaces; the parent compares them bit for
bit with the host twin and reads from the debug lines (PYDEM_COND_DEBUG=2) WHICH engine ran.  After a child that died by a
signal or ran into its time limit no further child is started.

The routes, as reached (defaults: launches per sweep `wl` while the list is longer than 8192 cells, else resident
workgroups `coop` for up to 512 sweeps; from the second look on, with at most 16384 cells listed, passes of 16 sweeps):
  default_route  16900-cell list: wl x 32, passes from sweep 33, three zigzags stop in mid-pass;
  zig_family     12234-cell list (the plain 96 x 96 lake is there for that): wl x 32, passes from sweep 33, 24 zigzags stop
                 all over the passes;
  long_zigzag    1058-cell list: coop x 512, passes from sweep 513; the outlet distance stops in the last sweep of the
                 first pass, the uphill distance in the first sweep of the second;
  centre_seeds   10368-cell list: wl x 32, passes from sweep 33, both lakes still sweeping from their centre cells;
  the others     coop to the end (stops before sweep 513) with no environment set, passes from 33 with the resident and
                 the one-workgroup kernel off (edge_lakes: the seeds on the tile edge, windows that reach outside the tile).
(A scratch build of the library can be put under these tests with PYDEM_TEST_LIB=<path>: the children load it instead.
Three planted mistakes were checked that way: the repeat run skipped, `done[r] = s0 + j + 1` in flat_accept_rows, `jlh`
from `P.s0 + T`.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flat_fields as F
from _flat_engines_worker import RUNS, run_key

pytestmark = pytest.mark.gpu

PLAIN = {'PYDEM_FLAT_COOP': '0', 'PYDEM_FLAT_SMALL': '0'}          # launches per sweep, then the passes, whatever the list length
SETTINGS = {
    'defaults': {},
    'wl_then_batch': PLAIN,
    'batch_T1': dict(PLAIN, PYDEM_FLAT_BATCH_T='1'),
    'batch_T5': dict(PLAIN, PYDEM_FLAT_BATCH_T='5'),
    'batch_8_regions': dict(PLAIN, PYDEM_FLAT_BATCH_REGIONS='8'),
    'single_sweeps': dict(PLAIN, PYDEM_FLAT_BATCH='0'),
    'one_workgroup': {'PYDEM_FLAT_COOP': '0'},
}
KNOBS = ('PYDEM_FLAT_COOP', 'PYDEM_FLAT_COOP_WG', 'PYDEM_FLAT_COOP_XCD', 'PYDEM_FLAT_COOP_MIN', 'PYDEM_FLAT_SMALL', 'PYDEM_FLAT_BATCH',
         'PYDEM_FLAT_BATCH_T', 'PYDEM_FLAT_BATCH_REGIONS')
CHILD_TIMEOUT = 120

_runs = {}
_dead = []


def _child(setting, tmp):
    """Surfaces and debug lines (per run) of one setting; every setting runs once per session."""
    if setting in _runs:
        return _runs[setting]
    if _dead:
        pytest.fail("not started: the child of %r died (%s)" % _dead[0])
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SETTINGS[setting], PYDEM_COND_DEBUG='2')
    out = os.path.join(str(tmp), setting + '.npz')
    try:
        r = subprocess.run([sys.executable, os.path.join(here, '_flat_engines_worker.py'), out], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append((setting, "time limit"))
        raise
    if r.returncode < 0:
        _dead.append((setting, "signal %d" % -r.returncode))
    assert r.returncode == 0 and 'FLAT-ENGINES-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lines = {}
    key = None
    for line in r.stderr.splitlines():
        if line.startswith('FLATFIELD '):
            key = line.split()[1]
            lines[key] = []
        elif key is not None and line.startswith('fill_flats:'):
            lines[key].append(line)
    with np.load(out) as d:
        _runs[setting] = ({k: d[k] for k in d.files}, lines)
    return _runs[setting]


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp('flat_engines')


@pytest.fixture(scope='module')
def want():
    """The host twin on every field, once."""
    from pydem_amd import conditioning as C
    res = {}
    for f in F.all_fields():
        for dtype, area in RUNS:
            z = f.z.astype(dtype)
            res[run_key(f.name, dtype, area)] = C.fill_flats(z) if area is None else C.fill_flats(z, area)
    return res


PASSES = re.compile(r'fill_flats: (\d+) passes of (\d+) sweeps from sweep (\d+), (\d+) ran again')
LOOK = re.compile(r'fill_flats: sweep (\d+), list (\d+) \(after a (\w+) look\)')


def _passes(lines):
    """(passes, sweeps per pass, first sweep, passes that ran again) of the run, or None when no pass ran."""
    got = [tuple(int(v) for v in m.groups()) for m in map(PASSES.match, lines) if m]
    assert len(got) <= 1
    return got[0] if got else None


def _looks(lines):
    return [(int(m.group(1)), int(m.group(2)), m.group(3)) for m in map(LOOK.match, lines) if m]


def _runs_of(name):
    return [run_key(name, dtype, area) for dtype, area in RUNS]


def check_defaults(lines):
    for name in ('default_route', 'zig_family', 'centre_seeds'):
        for key in _runs_of(name):
            looks, p = _looks(lines[key]), _passes(lines[key])
            assert [(s, e) for s, _, e in looks] == [(33, 'wl')] and p is not None and p[1:3] == (16, 33), (key, lines[key])
            assert p[3] >= 1 or name == 'centre_seeds', (key, lines[key])      # zigzags stop in mid-pass: passes ran again
    for key in _runs_of('long_zigzag'):
        looks, p = _looks(lines[key]), _passes(lines[key])
        assert [(s, e) for s, _, e in looks] == [(513, 'coop')] and p is not None and p[1:3] == (16, 513), (key, lines[key])
        assert p[0] >= 2 and p[3] >= 1, (key, lines[key])         # (the uphill distance stops in the first sweep of the second pass)
    for name in ('zigzag_k30_v3', 'zigzag_k40_v5', 'zigzag_k30_v4_apart20', 'edge_lakes'):
        for key in _runs_of(name):
            assert _passes(lines[key]) is None and {e for _, _, e in _looks(lines[key])} == {'coop'}, (key, lines[key])


def check_wl_then_batch(lines, T=16, repeats=True):
    for f in F.all_fields():
        for key in _runs_of(f.name):
            looks, p = _looks(lines[key]), _passes(lines[key])
            assert [(s, e) for s, _, e in looks] == [(33, 'wl')] and p is not None and p[1:3] == (T, 33), (key, lines[key])
            if not repeats:
                assert p[3] == 0, (key, lines[key])
            assert not any('deferred' in line for line in lines[key])
    if repeats:
        for name in ('zig_family', 'default_route', 'zigzag_k30_v3', 'zigzag_k40_v5', 'zigzag_k30_v4_apart20'):
            for key in _runs_of(name):
                assert _passes(lines[key])[3] >= 1, (key, lines[key])


def check_8_regions(lines):
    for key in _runs_of('zig_family'):
        deferred = [line for line in lines[key] if 'deferred' in line]
        assert deferred and ' 25 regions still sweeping, 8 table rows' in deferred[0], (key, lines[key])
        assert _passes(lines[key]) is not None                    # ... and the passes take over once few enough regions are left
    for key in _runs_of('default_route'):                         # four regions: nothing to defer
        assert not any('deferred' in line for line in lines[key]) and _passes(lines[key])[2] == 33


def check_single_sweeps(lines):
    for key, ls in lines.items():
        assert _passes(ls) is None and {e for _, _, e in _looks(ls)} == {'wl'}, (key, ls)
    assert max(s for s, _, _ in _looks(lines[run_key('long_zigzag', 'float64', 0.0)])) > 529


def check_one_workgroup(lines):
    for name in ('zigzag_k30_v3', 'zigzag_k40_v5', 'zigzag_k30_v4_apart20', 'edge_lakes'):
        for key in _runs_of(name):
            assert _looks(lines[key])[0][2] == 'small', (key, lines[key])
    for key in _runs_of('long_zigzag'):                           # 256 sweeps of one workgroup, then the passes
        assert _looks(lines[key])[0][::2] == (257, 'small') and _passes(lines[key])[2] == 257, (key, lines[key])
    for key in _runs_of('default_route'):
        assert _looks(lines[key])[0][2] == 'wl'


CHECKS = {'defaults': check_defaults, 'wl_then_batch': check_wl_then_batch,
          'batch_T1': lambda lines: check_wl_then_batch(lines, T=1, repeats=False),
          'batch_T5': lambda lines: check_wl_then_batch(lines, T=5),
          'batch_8_regions': check_8_regions, 'single_sweeps': check_single_sweeps, 'one_workgroup': check_one_workgroup}


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_engines_match_the_host_twin(setting, tmp, want):
    got, lines = _child(setting, tmp)
    assert sorted(got) == sorted(want)
    bad = ["%s: %d cells differ" % (k, int((got[k] != want[k]).sum())) for k in sorted(want)
           if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]
    assert not bad, "%s: %s" % (setting, "; ".join(bad))
    CHECKS[setting](lines)


def test_all_settings_give_the_same_bits(tmp):
    first, _ = _child('defaults', tmp)
    for setting in SETTINGS:
        got, _ = _child(setting, tmp)
        for k in first:
            assert np.array_equal(got[k], first[k]), (setting, k)
