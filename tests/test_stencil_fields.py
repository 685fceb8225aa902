"""The designed-facet kit (tests/stencil_fields.py) held to its own claims, without a device: that the fields reach the
places of the stencil's arithmetic they are built for (coverage, asserted), and that the CPU oracle -- the restated reference
-- itself passes on every designed cell what tests/test_gpu_stencil_bits.py asks of the kernels.  No designed cell is left
out of a check: where the oracle disagrees with the design, the design is what gets fixed."""
import math

import numpy as np
import pytest

import stencil_fields as SF
from flowgraph_kit import assert_same_bits
from stencil_fields import CARDINAL, DIAGONAL, INTERIOR, TIE, L

INTERIOR_FIELDS = [lambda s=s: SF.ratio_field(s) for s in SF.SCALES] + [SF.swapped_field, SF.tie_field, SF.quotient_field]


def _fields(dtype):
    return SF.float64_fields() if dtype == 'float64' else SF.float32_fields()


def _interior_cells(fields):
    """(s1, s2, d1, d2, k) of the interior winners (ties excluded) of the fields, concatenated"""
    out = []
    for f in fields:
        e = f.expected()
        sel = e['kind'] == INTERIOR
        out.append([e['s1'][sel], e['s2'][sel], e['d1'][sel], e['d2'][sel], f.k[sel]])
    return [np.concatenate(x) for x in zip(*out)]


# ---- coverage -------------------------------------------------------------------------------------------------------------
def test_every_table_entry_with_and_without_swap():
    s1, s2, _, _, _ = _interior_cells(SF.float64_fields())
    kf, swap = SF.table_index(s1, s2)
    for want_swap in (False, True):
        seen = set(kf[swap == want_swap].tolist())
        assert seen == set(range(17)), (want_swap, sorted(set(range(17)) - seen))


@pytest.mark.parametrize('scale', SF.SCALES)
def test_ratios_either_side_of_every_index_switch(scale):
    """within 2 spacings of each (k + 1/2) / 16, below and above it, on every facet -- as the ratio of the slopes the
    reference forms from the stored elevations, not of the ones the patch was designed with"""
    f = SF.ratio_field(scale)
    e = f.expected()
    q = e['s2'] / e['s1']
    assert (e['kind'] == INTERIOR).mean() > 0.98 and (q <= 1).all()      # (1 - 2^-53 may come out as a tie, or go to the facet across the diagonal)
    for facet in range(8):
        qk = q[f.k == facet]
        for k in range(1, 16):
            h = (k + 0.5) / 16
            off = (qk.astype(L) - L(h)) / L(np.spacing(h))
            assert ((off < 0) & (off >= -2)).any() and ((off > 0) & (off <= 2)).any(), (scale, facet, k)
            assert np.abs((qk - k / 16) / np.spacing(k / 16)).min() <= 2, (scale, facet, k)


def test_swapped_ratios_near_every_index_switch():
    """the `swap` branch: min / max of the realised slopes on either side of each (k + 1/2) / 16 that the ratios name (k = 1 .. 15)"""
    s1, s2, _, _, _ = _interior_cells([SF.swapped_field()])
    sw = s2 > s1
    assert sw.sum() > 500
    ratio = s1[sw] / s2[sw]
    for k in range(1, 16):
        h = (k + 0.5) / 16
        off = (ratio.astype(L) - L(h)) / L(np.spacing(h))
        assert ((off < 0) & (off >= -2)).any() and ((off > 0) & (off <= 2)).any(), k


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_all_facets_in_every_field(dtype):
    for f in _fields(dtype):
        assert set(f.k.tolist()) == set(range(8)), f.name
        assert len(set(zip(f.i.tolist(), f.j.tolist()))) == f.i.size, f.name


def test_both_spacing_families_with_unequal_spacings_and_swap():
    s1, s2, d1, d2, k = _interior_cells([SF.swapped_field()])
    fam_a = np.isin(k, SF.FAMILY_A)
    for fam in (fam_a, ~fam_a):
        assert (fam & (d1 != d2)).any() and (fam & (d1 != d2) & (s2 > s1)).any() and (fam & (d1 != d2) & (s2 < s1)).any()
    e = SF.tie_field().expected()
    fam_a = np.isin(SF.tie_field().k, SF.FAMILY_A)
    assert (fam_a & (e['d1'] != e['d2'])).any() and (~fam_a & (e['d1'] != e['d2'])).any()


def test_all_four_scales():
    got = sorted(float(np.abs(SF.ratio_field(s).expected()['s1']).max()) for s in SF.SCALES)
    assert np.allclose(got, sorted(SF.SCALES), rtol=1e-15, atol=0)
    assert min(SF.SCALES) == 2.0 ** -470 and max(SF.SCALES) == 2.0 ** 470


def test_cardinal_diagonal_interior_and_tied_winners():
    kinds = np.concatenate([f.expected()['kind'] for f in SF.float64_fields()])
    for kind in (CARDINAL, DIAGONAL, INTERIOR, TIE):
        assert (kinds == kind).sum() >= 100, kind
    q = SF.quotient_field()
    e = q.expected()
    assert set(e['kind'].tolist()) == {CARDINAL, DIAGONAL}
    for facet in range(8):
        assert (e['kind'][q.k == facet] == DIAGONAL).any(), facet
    assert set(q.k[e['kind'] == CARDINAL].tolist()) == {0, 1, 3, 4, 5, 7}          # (2 and 6 never win a cardinal edge: 1 and 5 come first)
    diag = e['kind'] == DIAGONAL
    assert (diag & (e['s1'] <= 0)).any() and (diag & (e['s1'] > 0)).any()           # both ways into the state
    assert (e['s2'][e['kind'] == CARDINAL] < 0).any() and (e['s2'][e['kind'] == CARDINAL] == 0).any()
    # every awkward spacing divides some designed numerator, as dX, dY and inside a hypotenuse
    for d in SF.AWKWARD:
        assert (e['d1'][e['kind'] == CARDINAL] == d).any(), d
        assert ((e['d1'][diag] == d) | (e['d2'][diag] == d)).any(), d


def test_ties_are_exact():
    f = SF.tie_field()
    e = f.expected()
    assert np.isin(e['kind'], (TIE, DIAGONAL)).all() and (e['kind'] == TIE).sum() >= 256     # (DIAGONAL: the facet across the diagonal takes the cell with the same angle)
    assert np.array_equal(e['s2'] * e['d1'], e['s1'] * e['d2'])
    assert np.array_equal(e['s2'].astype(L) * e['d1'].astype(L), e['s1'].astype(L) * e['d2'].astype(L))      # ... and not only after rounding
    pairs = set(zip(f.dX[np.where(f.k < 4, f.i - 1, f.i)].tolist(), f.dY[np.where(f.k < 4, f.i - 1, f.i)].tolist()))
    assert pairs == set((float(a), float(b)) for a, b in SF.TIE_PAIRS)
    for pair in pairs:
        here = (f.dX[np.where(f.k < 4, f.i - 1, f.i)] == pair[0]) & (f.dY[np.where(f.k < 4, f.i - 1, f.i)] == pair[1])
        assert set(f.k[here].tolist()) == set(range(8)), pair


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_slopes_stay_inside_the_documented_window(dtype):
    for f in _fields(dtype):
        e = f.expected()
        for s in (e['s1'], e['s2'], e['sd']):
            nz = np.abs(s[s != 0])
            assert nz.min() >= 2.0 ** -480 and nz.max() <= 2.0 ** 480, f.name
        zmax = np.abs(f.z.astype(np.float64)).max()
        assert zmax < 2.0 ** 481 and (zmax / min(f.dX.min(), f.dY.min())) ** 2 < 2.0 ** 1000, f.name     # no square of any slope of the field overflows
        if dtype == 'float32':
            assert f.z.dtype == np.float32
            assert np.abs(f.z[f.z != 0]).min() >= 2.0 ** -100                     # (no float32 subnormal difference anywhere near)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_no_cell_of_any_field_leaves_the_window(dtype):
    """filler cells included, and with the markers in (a NaN region un-flags flats next to it): every magnitude the reference
    stores is -1, inf next to a huge marker, or within [2^-480, 2^480] -- its square is normal"""
    fields = _fields(dtype) + ([SF.marked(SF.ratio_field(s), v) for s in SF.SCALES for v in (np.nan, 2.0 ** 600)] if dtype == 'float64' else [])
    for f in fields:
        mag, _ = _oracle(f)
        pos = mag[(mag > 0) & np.isfinite(mag)]
        assert not np.isnan(mag).any() and (mag[mag <= 0] == -1).all(), f.name
        assert pos.min() >= 2.0 ** -480 and pos.max() <= 2.0 ** 480, (f.name, pos.min(), pos.max())
        assert np.isinf(mag).sum() == (2 * f.shape[0] if f.marker == 2.0 ** 600 else 0), f.name


# ---- layout: the places of the marching kernel the designed cells fall on --------------------------------------------------
@pytest.mark.parametrize('make', INTERIOR_FIELDS + [lambda: SF.ratio_field(1.0, 'float32'), lambda: SF.quotient_field('float32')])
def test_strips_chunks_and_bands(make):
    f = make()
    n, m = f.shape
    assert n <= 260 and m <= 200
    strips = SF.strip_columns(m)
    assert len(strips) > 1 and (m - 2) % SF.STRIP != 0                             # more than one strip, a ragged last one
    rows = SF.chunk_rows(n, m)
    chunks = SF.cdiv(n - 2, rows)
    assert rows == 16 and chunks >= 3
    first, last, parity = set(), set(), set()
    for i in set(f.i.tolist()):
        c, q = divmod(i - 1, rows)
        end = min(rows, n - 2 - c * rows) - 1
        if q == 0:
            first.add(c)
        if q == end:
            last.add(c)
        parity.add(q & 1)
    assert first and last and parity == {0, 1}                                     # the first band of a wavefront, its last one, odd and even ones
    for lo, hi in strips:
        assert ((f.j >= lo + 1) & (f.j <= hi - 2)).any()                           # designed cells in every strip
    assert len(f.spare_cols) == len(strips)
    for c, (lo, hi) in zip(f.spare_cols, strips):
        assert lo <= c < hi
        assert np.abs(f.j - c).min() >= 3                                          # two columns from the cells of any patch


@pytest.mark.parametrize('value', [np.nan, 2.0 ** 600])
def test_marked_field_reaches_every_band_and_no_designed_cell(value):
    base = SF.ratio_field(1.0)
    f = SF.marked(base, value)
    hit = np.isnan(f.z) if np.isnan(value) else f.z == value
    for lo, hi in SF.strip_columns(f.shape[1]):
        assert hit[:, lo:hi].any(axis=1).all()                                     # a marker in every row the strip reads: every band takes the exact path
    near = np.zeros(f.shape, bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            near[f.i + di, f.j + dj] = True
    assert not (hit & near).any()
    e0, e1 = base.expected(), f.expected()
    for key in ('s1', 's2', 'mag', 'direction'):
        assert np.array_equal(e0[key], e1[key])


# ---- the reference stays inside the bars -----------------------------------------------------------------------------------
def _oracle(f):
    from oracle import oracle as O
    mag, direction = O.slopes_directions(f.z, f.dX, f.dY)        # (a float32 field goes in as float32: the oracle then subtracts in float32)
    return mag, direction


def direction_error(direction, e, ulps_r, ulps_direction):
    """|direction - longdouble value| as a fraction of ulps_r spacing(r) + ulps_direction spacing(direction): the error of an
    arctangent good to ulps_r spacings of its own value r, plus the rounding of r a1 + a0 pi/2 (where that sum cancels, in
    pi/2 - r with r near pi/2, the spacing of the direction is far below r's)"""
    sp_r = np.spacing(np.abs(e['r']).astype(np.float64)).astype(L)
    sp_d = np.spacing(np.abs(e['direction']).astype(np.float64)).astype(L)
    return np.abs(direction.astype(L) - e['direction']) / (ulps_r * sp_r + ulps_direction * sp_d)


def assert_designed_facet(direction, e, what):
    """the direction lies in the sector of the designed facet, a0 pi/2 .. a0 pi/2 + a1 theta (its ends to within their own rounding)"""
    base = e['a0'].astype(np.float64) * np.pi / 2
    end = base + e['a1'] * e['theta'].astype(np.float64)
    lo, hi = np.minimum(base, end), np.maximum(base, end)
    slack = 2 * np.spacing(hi)
    bad = (direction < lo - slack) | (direction > hi + slack)
    assert not bad.any(), "%s: %d designed cells went to another facet" % (what, bad.sum())


@pytest.mark.parametrize('dtype,idx', [('float64', q) for q in range(10)] + [('float32', q) for q in range(8)])
def test_oracle_passes_on_every_designed_cell(dtype, idx):
    assert len(_fields(dtype)) == (10 if dtype == 'float64' else 8)              # (the cases above name every field)
    f = _fields(dtype)[idx]
    e = f.expected()
    mag, direction = _oracle(f)
    m_cells, d_cells = mag[f.i, f.j], direction[f.i, f.j]
    assert_same_bits(m_cells, e['mag'], f.name + ' mag')
    assert_designed_facet(d_cells, e, f.name)
    # glibc's arctangent to within 3/4 of a spacing of r (0.51 measured), the final addition rounds once
    err = direction_error(d_cells, e, 0.75, 0.5)
    print('%s: %d designed cells, oracle direction at most %.3f of 0.75 spacing(r) + 0.5 spacing(direction)' % (f.name, f.i.size, float(err.max())))
    assert err.max() <= 1.0, f.name
    tie = e['kind'] == TIE
    if f is SF.tie_field():
        assert_same_bits(d_cells, (e['theta'].astype(np.float64) * e['a1'] + e['a0'].astype(np.float64) * np.pi / 2), f.name + ' = table angle of the winner')
    if tie.any():
        table = np.array([math.atan2(b, a) for a, b in zip(e['d1'][tie], e['d2'][tie])])
        assert_same_bits(d_cells[tie], table * e['a1'][tie] + e['a0'][tie].astype(np.float64) * np.pi / 2, f.name + ' tie = table angle')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_perimeter_copy_rule_brings_nothing(dtype):
    """the interior neighbour a border cell would copy from holds no direction inside the rule's open interval (it drains along
    the edge, or is a flat), the diagonal neighbour of a corner is a flat, and the plateau inside is flat"""
    for pair in SF.PERIMETER_PAIRS:
        f = SF.perimeter_field(*pair, dtype=dtype)
        n, m = f.shape
        mag, direction = _oracle(f)
        assert (mag[3:n - 3, 3:m - 3] == -1).all()
        corners = 0
        for i, j in zip(f.i.tolist(), f.j.tolist()):
            ii = 1 if i == 0 else (n - 2 if i == n - 1 else i)
            jj = 1 if j == 0 else (m - 2 if j == m - 1 else j)
            d = direction[ii, jj]
            if (i in (0, n - 1)) and (j in (0, m - 1)):
                corners += 1
                assert mag[ii, jj] == -1 and d == -1
            elif i == 0:
                assert not (0 < d < np.pi)
            elif i == n - 1:
                assert not (np.pi < d < 2 * np.pi)
            elif j == 0:
                assert not (np.pi / 2 < d < 3 * np.pi / 2)
            else:
                assert not (d < np.pi / 2 or d > 3 * np.pi / 2) or d == -1
        assert corners == 4
