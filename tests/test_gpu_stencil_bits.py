"""The stencil's own arithmetic (csrc/stencil.hip: div_row, div_pos, sqrt_window, atan2_pos / atan2_pos_fast, the table-angle
override of exact ties) held to what its comments claim, on the designed facets of tests/stencil_fields.py -- the places
where that arithmetic can go wrong, which random terrain under a relative tolerance of 1e-11 never shows.

The bars, for every designed cell of every field and on every path of the kernel:
  flats      equal to the oracle's over the whole field;
  mag        the bits of np.sqrt(s1 * s1 + s2 * s2) (|s1|, |sd| for a cardinal / diagonal winner) formed from the stored
             elevations -- the quotients and the root are "correctly rounded like `/`" -- and the oracle's bits over the whole
             field, filler cells included;
  direction  the oracle's bits where the slopes are in the exact ratio of the spacings (the table angle);
             elsewhere |direction - longdouble value| <= 2 spacing(r) + spacing(direction), r = arctan2(s2, s1): the kernel
             states 1.5 ulp of r for its arctangent (a simulation of atan2_pos_fast in exact arithmetic: 1.35, glibc: 0.51),
             the addition of a0 pi/2 rounds once more.  Derived, not tuned.

The paths: the marching kernel with its mask algebra (default), on its exact path for the whole tile (PYDEM_STENCIL_EXACT=1,
read when the spacing is set) and band by band (a NaN or 2^600 in every row of every strip), the store split
(PYDEM_STENCIL_SPLIT=1, read per launch); in child processes, one at a time, the LDS tile kernel (PYDEM_STENCIL=tile) and the
128-VGPR build (PYDEM_STENCIL_OCC=4), both read once per process.  The perimeter kernel runs with each of them.

Each case prints the worst arctangent it saw, in spacings of r (DESIGN.md section 4.1 carries the numbers)."""
import functools
import re

import numpy as np
import pytest

import flowgraph_kit as K
import stencil_fields as SF
from stencil_fields import INTERIOR, TIE, L

pytestmark = pytest.mark.gpu

ULPS_R, ULPS_DIRECTION = 2.0, 1.0


def fields_of(dtype):
    return SF.float64_fields() if dtype == 'float64' else SF.float32_fields()


def marked_fields():
    return [SF.marked(SF.ratio_field(s), v) for s in SF.SCALES for v in (np.nan, 2.0 ** 600)]


@functools.lru_cache(maxsize=None)
def oracle_of(field):
    """(mag, direction, flats) of the CPU oracle, computed once per field and process and never changed"""
    from oracle import oracle as O
    o = O.OracleDEM(field.z, dX=field.dX, dY=field.dY)
    o.calc_slopes_directions()
    out = (o.mag, o.direction, o.flats.astype(bool))
    for a in out:
        a.setflags(write=False)
    return out


def device_of(field):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=field.z.copy(), fill_flats=False, drain_pits_path=False, **field.spacing)
    mag, direction = dp.calc_slopes_directions()
    return np.array(mag), np.array(direction), np.array(dp.flats, bool)


def check(field, path):
    """every bar of the module on one field; returns (sha256 of mag, worst arctangent error in spacings of r, worst direction
    error as a fraction of its bound)"""
    e = field.expected()
    omag, odir, oflats = oracle_of(field)
    mag, direction, flats = device_of(field)
    what = '%s, %s' % (field.name, path)
    i, j = field.i, field.j
    problems = []                                                                # every bar is looked at before the case fails

    def bar(fn, *args):
        try:
            fn(*args)
        except AssertionError as err:
            problems.append(str(err))
    if not np.array_equal(flats, oflats):
        problems.append('flats, %s: %d cells differ' % (what, (flats != oflats).sum()))
    assert not oflats[i, j].any(), what
    bar(K.assert_same_bits, mag[i, j], e['mag'], 'mag of the designed cells, ' + what)
    bar(K.assert_same_bits, mag, omag, 'mag of the whole field, ' + what)
    d = direction[i, j]
    tie = (e['kind'] == TIE) | (field is SF.tie_field())          # (every cell of the tie field: where the facet across the diagonal takes it, its table angle)
    if tie.any():
        bar(K.assert_same_bits, d[tie], odir[i, j][tie], 'direction of the exact ties, ' + what)
    err = np.abs(d.astype(L) - e['direction'])
    sp_r = np.spacing(np.abs(e['r']).astype(np.float64)).astype(L)
    sp_d = np.spacing(np.abs(e['direction']).astype(np.float64)).astype(L)
    frac = (err / (ULPS_R * sp_r + ULPS_DIRECTION * sp_d))[~tie]
    # the arctangent alone: interior winners of facet 0, whose direction IS r (a0 = 0, a1 = 1: nothing is added)
    pure = (e['kind'] == INTERIOR) & (e['k_win'] == 0)
    worst_r = float((err[pure] / sp_r[pure]).max()) if pure.any() else 0.0
    worst = float(frac.max()) if frac.size else 0.0
    print('%s: %d designed cells, arctangent off by at most %.3f spacing(r) on facet 0, direction at most %.3f of its bound'
          % (what, i.size, worst_r, worst))
    if not (frac <= 1.0).all():
        problems.append('direction, %s: %d designed cells beyond 2 spacing(r) + spacing(direction), worst %.3f of it' % (what, (~(frac <= 1.0)).sum(), worst))
    assert not problems, '; '.join(problems)
    return K.bits(mag), worst_r, worst


def check_all(fields, path):
    rows = [(f.name,) + check(f, path) for f in fields]
    print('%s: worst arctangent %.3f spacing(r), worst direction %.3f of the bound, %d fields'
          % (path, max(r[2] for r in rows), max(r[3] for r in rows), len(rows)))
    return rows


# ---- in process ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_march_mask_algebra(dtype):
    check_all(fields_of(dtype), 'march, mask algebra')


def test_march_exact_for_the_whole_tile(monkeypatch):
    monkeypatch.setenv('PYDEM_STENCIL_EXACT', '1')
    check_all(SF.float64_fields(), 'march, exact (whole tile)')


def test_march_exact_band_by_band():
    """a NaN / 2^600 in a spare patch column of every strip, in every row: every band of every wavefront takes the exact path,
    the window test finds it band by band; the expected values of the designed cells are those of the plain field"""
    fields = marked_fields()
    for f in fields:
        hit = np.isnan(f.z) | (f.z == 2.0 ** 600)
        for lo, hi in SF.strip_columns(f.shape[1]):
            assert hit[:, lo:hi].any(axis=1).all(), f.name                    # every band of every strip holds such a cell
        assert np.abs(f.j[:, None] - np.array(f.spare_cols)[None, :]).min() >= 3
        base = SF.ratio_field(SF.SCALES[fields.index(f) // 2]).expected()
        assert np.array_equal(f.expected()['mag'], base['mag']) and np.array_equal(f.expected()['direction'], base['direction'])
    check_all(fields, 'march, exact (band by band)')


def test_march_store_split(monkeypatch):
    monkeypatch.setenv('PYDEM_STENCIL_SPLIT', '1')
    check_all(SF.float64_fields(), 'march, store split')


# ---- switches read once per process: one child each, one at a time -----------------------------------------------------------
CHILD = """
import test_gpu_stencil_bits as T
for dtype in %r:
    for row in T.check_all(T.fields_of(dtype), %r):
        print('BITS|%%s|%%s|%%.6f|%%.6f' %% row)
print('CHILD-OK')
"""


def _child(env, dtypes, path):
    r = K.run_child(CHILD % (dtypes, path), env=env, timeout=300)
    got = {m[0]: m[1:] for m in re.findall(r'^BITS\|(.*)\|([0-9a-f]{64})\|([0-9.]+)\|([0-9.]+)$', r.stdout, re.M)}
    fields = [f for dtype in dtypes for f in fields_of(dtype)]
    assert sorted(got) == sorted(f.name for f in fields), r.stdout[-2000:]
    for f in fields:
        sha, worst_r, worst = got[f.name]
        assert sha == K.bits(oracle_of(f)[0]), f.name
        assert float(worst) <= 1.0, f.name
    print('\n'.join(line for line in r.stdout.splitlines() if 'spacing(r)' in line))


def test_lds_tile_kernel():
    _child({'PYDEM_STENCIL': 'tile'}, ('float64', 'float32'), 'LDS tile kernel')


def test_128_vgpr_build():
    _child({'PYDEM_STENCIL_OCC': '4'}, ('float64',), 'march, 128 VGPRs')
