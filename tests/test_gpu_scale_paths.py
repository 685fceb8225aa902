"""The schedules the per-tile kernels only take on large tiles, cell by cell against the CPU oracle:

  A  the marching stencil (csrc/stencil.hip launch_stencil) at chunk heights of 128, 64 and 32 rows, with a spacing that
     changes from row to row, terraces (exact ties), a plateau and NaN specks in some chunks only.  The stencil is local, so
     the oracle runs on horizontal slabs of whole chunks plus two halo rows: the first chunks, two in the middle, the ragged
     last ones.
  B  the UCA sweep (csrc/uca.hip stage_sweep) on the 8192 x 8192 bench tile: full passes with more tiles than the persistent
     grid, listed passes whose wavefronts take several list entries (grid-stride loop), batches of 8 and 16 passes between
     two looks of the host, the two-level solve with 16 pool regions after numeric listed passes.  The schedule switches are
     read once per process, so each schedule runs in a child process, one at a time, against one oracle run of the parent.
  C  the widest tile the sweep accepts, 3 x (2^22 - 1), and the refusal one column past it.

Bars of tests/test_gpu_parity.py: integer fields and masks bit for bit, float fields within RTOL, the same NaN pattern; pit
pairs and weights as tests/test_gpu_capacity_edges.py holds them.  Each case also shows that the device took its branch."""
import os
import re
import shutil
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

from test_gpu_capacity_edges import _check_parity
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cdiv(a, b):
    return -(-a // b)


def check_full_path(dp, o, twi):
    """every field of the full path against an oracle run (OracleDEM after calc_twi, or its fields loaded back)"""
    _check_parity(dp, o, twi)
    _close(dp.direction, o.direction, 'direction')
    _close(dp.proportion, o.proportion, 'proportion')
    _close(dp.twi, o.twi, 'twi attr')


# --- A: the marching stencil at chunk heights above 16 rows -------------------------------------------------------------

MARCH_ROWS = 128        # csrc/stencil.hip MARCH_ROWS
STRIP = 62              # output columns of one wavefront strip


def chunk_rows(n, m):
    """csrc/stencil.hip launch_stencil: rows per chunk halve from MARCH_ROWS while the tile would give the chip fewer than 12288
    wavefronts, down to 16"""
    strips = cdiv(m - 2, STRIP)
    rows = MARCH_ROWS
    while rows > 16 and strips * cdiv(n - 2, rows) < 12288:
        rows >>= 1
    return rows


STENCIL_CASES = [(128, (7855, 12357), 'float64'), (128, (7855, 12357), 'float32'),
                 (64, (9000, 6190), 'float64'), (32, (9000, 3090), 'float32')]


def _spacing(n):
    i = np.arange(n, dtype=np.float64)
    dX2 = 25.0 + 0.004 * i + 0.5 * np.sin(0.37 * i)
    dY2 = 31.0 - 0.002 * i + 0.3 * np.cos(0.23 * i)
    return dict(dX=dX2[:-1] + 0.01, dY=dY2[:-1] - 0.01, dX2=dX2, dY2=dY2)


def _chunk_span(c, rows, n):
    """output rows [lo, hi) of chunk c (the first output row is 1; the last chunk ends at n - 1)"""
    return 1 + c * rows, min(1 + (c + 1) * rows, n - 1)


def _stencil_slabs(n, rows):
    """row ranges compared with the oracle: two whole chunks each -- the first two (with the tile's first row), two in the
    middle, the last two (the ragged one and the tile's last row)"""
    chunks = cdiv(n - 2, rows)
    mid = chunks // 2
    return [(0, _chunk_span(1, rows, n)[1]), (_chunk_span(mid, rows, n)[0], _chunk_span(mid + 1, rows, n)[1]),
            (_chunk_span(chunks - 2, rows, n)[0], n)]


def _stencil_terrain(n, m, rows, seed):
    """fractal (a 1024-row block repeated down the tile, on a ramp), integer terraces and a plateau across chunk boundaries in
    every slab, NaN specks in the second chunk and the last one only; returns z and the chunks that hold NaN"""
    from oracle import oracle as O
    block = O.synth_fractal(1024, m, seed=seed, n_octaves=9, top_shift=8, zrange=300.0)
    z = np.tile(block, (cdiv(n, 1024), 1))[:n] + 0.01 * np.arange(n)[:, None]
    rng = np.random.default_rng(seed)
    chunks = cdiv(n - 2, rows)
    for lo, hi in _stencil_slabs(n, rows):
        b = (lo or 1) + rows                                                     # the chunk boundary inside the slab
        z[b - 20:b + 20, 100:700] = np.rint(z[b - 20:b + 20, 100:700])         # terraces: exact ties across the boundary
        z[b - 9:b + 7, 900:960] = z[b, 900]                                      # a plateau across it
        z[lo:hi, m - 50:] = np.rint(z[lo:hi, m - 50:] * 0.5)                    # ties in the ragged last strip
    nan_chunks = (1, chunks - 1)
    for c in nan_chunks:
        lo, hi = _chunk_span(c, rows, n)
        r = rng.integers(lo + 2, hi - 2, 6)
        q = rng.integers(2, m - 2, 6)
        z[r, q] = np.nan
        z[(lo + hi) // 2, m - 3] = np.nan                                        # in the ragged last strip
    return z, nan_chunks


@pytest.mark.parametrize('rows,shape,dtype', STENCIL_CASES, ids=['%d_rows_%s' % (c[0], c[2]) for c in STENCIL_CASES])
def test_stencil_tall_chunks_against_oracle(rows, shape, dtype):
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    n, m = shape
    # the branch: the restated rule gives this chunk height; the last strip and the last chunk are ragged
    assert chunk_rows(n, m) == rows, (shape, chunk_rows(n, m))
    assert (m - 2) % STRIP != 0 and (n - 2) % rows != 0
    z, nan_chunks = _stencil_terrain(n, m, rows, seed=rows + len(dtype))
    z = z.astype(dtype)
    sp = _spacing(n)
    dp = DEMProcessor(elev=z, fill_flats=False, drain_pits_path=False, **sp)
    dp.calc_slopes_directions()
    mag, direction, flats = np.asarray(dp.mag), np.asarray(dp.direction), np.asarray(dp.flats)
    del dp
    nan_rows = np.isnan(z).any(axis=1)
    for lo, hi in _stencil_slabs(n, rows):
        r0, r1 = max(lo - 2, 0), min(hi + 2, n)
        om, od = O.slopes_directions(z[r0:r1], sp['dX'][r0:r1 - 1], sp['dY'][r0:r1 - 1])
        of = O.flats_edges(np.asarray(z[r0:r1], np.float64), om, od).astype(bool)
        k0, k1 = lo - r0, hi - r0
        what = 'rows %d-%d of %dx%d %s (chunks of %d)' % (lo, hi, n, m, dtype, rows)
        _close(mag[lo:hi], om[k0:k1], 'mag, ' + what)
        _close(direction[lo:hi], od[k0:k1], 'direction, ' + what)
        assert np.array_equal(flats[lo:hi], of[k0:k1]), 'flats, ' + what
        assert (om[k0:k1] == -1).any() and (om[k0:k1] > 0).any(), what          # flats and slopes
    # bands next to a NaN are decided facet by facet, the others by mask algebra: the first and last slabs have both kinds
    (a0, a1), (b0, b1), (c0, c1) = _stencil_slabs(n, rows)
    assert nan_rows[a0:a1].any() and not nan_rows[b0:b1].any() and nan_rows[c0:c1].any()
    print('stencil %dx%d %s: chunks of %d rows, %d strips, %d chunks, NaN in chunks %s'
          % (n, m, dtype, rows, cdiv(m - 2, STRIP), cdiv(n - 2, rows), nan_chunks))


# --- B: the sweep's large-tile schedule at 8192^2 -----------------------------------------------------------------------

BIG = 8192
ORACLE_FIELDS = ('elev', 'mag', 'direction', 'flats', 'section', 'proportion', 'uca', 'edge_todo', 'edge_done', 'twi',
                 'pit_i', 'pit_j', 'pit_prop')


@pytest.fixture(scope='module')
def big_oracle(tmp_path_factory):
    """the oracle's full path on the bench generator's 8192^2 tile (seed 1), saved field by field for the children"""
    from oracle import oracle as O
    d = tmp_path_factory.mktemp('sweep8192')
    z = O.synth_fractal(BIG, BIG, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o = O.OracleDEM(z, dX=30.0, dY=30.0, drain_pits=True)
        o.calc_twi()
    for f in ORACLE_FIELDS:
        np.save(str(d / (f + '.npy')), np.asarray(getattr(o, f)))
    np.save(str(d / 'n_warn.npy'), np.asarray(o.n_warn))
    np.save(str(d / 'reseed_rounds.npy'), np.asarray(o.stats[0]))
    del o
    yield str(d)
    shutil.rmtree(str(d), ignore_errors=True)           # (3.4 GB)


def child_sweep(d):
    """(child process) the device's full path on the same tile against the saved oracle fields"""
    from pydem_amd import DEMProcessor
    o = types.SimpleNamespace(**{f: np.load(os.path.join(d, f + '.npy'), mmap_mode='r') for f in ORACLE_FIELDS})
    o.n_warn = int(np.load(os.path.join(d, 'n_warn.npy')))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor.from_synthetic((BIG, BIG), dict(seed=1), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False,
                                         drain_pits=True)
        twi = dp.calc_twi()
    assert np.array_equal(np.asarray(dp.elev), o.elev), "the device generator is not the oracle's"
    check_full_path(dp, o, twi)


def _sweep_log(err):
    """the PYDEM_SWEEP_DEBUG lines of one stage_sweep: listed after passes 1-2, the host's looks (pass, listed next) before the
    symbolic pass and after it, the symbolic pass and the two-level solve's counters"""
    lines = err.splitlines()
    first = [int(x) for x in re.findall(r'^tile passes 1-2: \d+ cells of \d+, (\d+) tiles listed$', err, re.M)]
    sym_at = next((k for k, l in enumerate(lines) if l.startswith('symbolic pass ')), len(lines))
    looks = [(k < sym_at, int(a), int(b)) for k, l in enumerate(lines)
             for a, b in re.findall(r'^listed tile pass (\d+): (\d+) tiles listed next', l)]
    two = re.findall(r'two-level solve: (\d+) symbolic tiles \((\d+) fell back to numeric visits\), \d+ outlets, \d+ symbolic cells, '
                     r'pool (\d+) of (\d+) doubles', err)
    assert len(first) == 1, err[-3000:]
    return dict(listed_after_2=first[0], symbolic_pass=sym_at < len(lines), looks=looks,
                two_level=tuple(int(x) for x in two[-1]) if two else None)


SWEEP_SCHEDULES = [('default', {}), ('numeric', {'PYDEM_SWEEP_SYM': '0'}), ('symbolic_after_2', {'PYDEM_SWEEP_SYM': '100000000'})]


def _check_schedule(name, L):
    """the branches the schedule took, from its debug lines.  (Batch sizes are reported, not asserted: they only decide how
    often the host looks, and a test must not depend on that.)"""
    looks_before = [lk for lk in L['looks'] if lk[0]]
    if name == 'default':
        # more than 8192 x 2 x 2 tiles listed: each wavefront of the capped grid of k_sweep_tiles_listed takes several entries
        assert L['listed_after_2'] > 32768, L
        assert looks_before, L                                                  # numeric listed passes first ...
        assert L['symbolic_pass'] and L['two_level'] and L['two_level'][0] > 0, L      # ... then symbolic tiles
    elif name == 'numeric':
        assert not L['symbolic_pass'] and L['two_level'] is None and L['looks'][-1][2] == 0, L
        left = [L['listed_after_2']] + [lk[2] for lk in L['looks'][:-1]]       # tiles listed when each batch was launched
        assert any(nl > 8192 for nl in left) and any(nl < 8192 for nl in left), left       # the grid shrank
        assert any(nl >= 2048 for nl in left) and any(nl < 2048 for nl in left), left      # batches of 8, then of 16
    else:
        assert not looks_before and L['symbolic_pass'], L                       # the symbolic pass right after pass 2
        assert L['two_level'][0] + L['two_level'][1] > 0 and L['two_level'][2] <= L['two_level'][3], L


def test_sweep_8192_schedules_against_oracle(big_oracle):
    """each schedule against the oracle; a child takes ~10 s, so one that runs for minutes has left cells to the re-seed
    replay (K5c) that the tile passes should have finished"""
    reseed = float(np.load(os.path.join(big_oracle, 'reseed_rounds.npy')))
    script = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_scale_paths as T\nT.child_sweep(%r)\nprint('SCALE-OK')\n"
              % (ROOT, os.path.join(ROOT, 'tests'), big_oracle))
    for name, env in SWEEP_SCHEDULES:
        r = subprocess.run([sys.executable, '-c', script], env=dict(os.environ, PYDEM_SWEEP_DEBUG='1', **env),
                           capture_output=True, text=True, timeout=180, cwd=ROOT)
        assert r.returncode == 0 and 'SCALE-OK' in r.stdout, (name, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
        if reseed <= 1:     # the oracle finished the tile without re-seeding: so must the device's tile passes
            assert 'circular drainage' not in r.stderr, (name, r.stderr[-3000:])
        L = _sweep_log(r.stderr)
        print('sweep 8192^2 %s: %d tiles listed after pass 2; (pass, listed next) at the looks before the symbolic pass %s, '
              'after it %s; two-level solve (symbolic tiles, fall-backs, pool used, pool) %s'
              % (name, L['listed_after_2'], [lk[1:] for lk in L['looks'] if lk[0]], [lk[1:] for lk in L['looks'] if not lk[0]],
                 L['two_level']))
        _check_schedule(name, L)


# --- C: the widest tile the sweep accepts ------------------------------------------------------------------------------

WIDEST = (1 << 22) - 1          # csrc/uca.hip stage_sweep refuses 2^22 columns and more


def test_widest_tile_against_oracle():
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    n, m = 3, WIDEST
    assert cdiv(m, 32) == 131072 and cdiv(m - 2, STRIP) == 67651          # one row of sweep tiles; stencil strips
    z = O.synth_fractal(n, m, seed=9, n_octaves=10, top_shift=9, zrange=200.0)
    z[:, 1000:3000] = np.rint(z[:, 1000:3000])
    sp = dict(dX=np.array([27.0, 29.0]), dY=np.array([31.0, 33.0]), dX2=np.array([26.0, 28.0, 30.0]), dY2=np.array([32.0, 30.0, 34.0]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o = O.OracleDEM(z, drain_pits=True, **sp)
        o.calc_twi()
        dp = DEMProcessor(elev=z, fill_flats=False, drain_pits_path=False, drain_pits=True, **sp)
        twi = dp.calc_twi()
    check_full_path(dp, o, twi)


def test_tile_one_column_too_wide_is_refused():
    from pydem_amd import DEMProcessor
    z = np.tile(np.linspace(100.0, 0.0, 1 << 22), (3, 1))
    z[1] += 1.0
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=False)
    with pytest.raises(RuntimeError, match='tiles wider than 4 194 303 columns are not supported'):
        dp.calc_uca()
