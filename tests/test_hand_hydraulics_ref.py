"""CPU tier: the numpy twin of pydem_hand_table (pydem_amd/hydraulics.py: hand_table_ref) and the hydraulic table made of its
integers (hydraulic_table) against closed forms.  Every designed plane has terms that are small dyadic numbers, so the fixed
point holds them exactly and the comparison is ==.  The GPU tier (test_gpu_hand_hydraulics.py) runs the same planes through the
device and compares with the twin; the builders here are shared with it."""
import numpy as np
import pytest

from pydem_amd import hydraulics as H
from pydem_amd.conditioning import fixed_point


# ---- the designed planes: dict(zone, hand, stages, dX2, dY2, mag, K) ---------------------------------------------------------
def case(zone, hand, stages, dX2=None, dY2=None, mag=None, K=None):
    zone = np.ascontiguousarray(zone, np.int32)
    n, m = zone.shape
    return dict(zone=zone, hand=np.ascontiguousarray(hand, np.float64), stages=np.asarray(stages, np.float64),
                dX2=np.full(n, 2.0) if dX2 is None else np.asarray(dX2, np.float64),
                dY2=np.full(n, 4.0) if dY2 is None else np.asarray(dY2, np.float64),
                mag=np.full((n, m), 0.75) if mag is None else np.ascontiguousarray(mag, np.float64),       # sqrt(1 + 0.75^2) = 1.25
                K=int(zone.max()) if K is None else K)


def uniform_case(shape=(6, 10)):
    """one zone, one value: every cell in bin 1 of [0.25, 0.5, 1.0]"""
    return case(np.ones(shape, np.int32), np.full(shape, 0.5), [0.25, 0.5, 1.0])


WEDGE_G, WEDGE_STAGES = 0.5, (0.5, 1.0, 2.0, 4.0, 8.0)


def wedge_case(shape, band, c0):
    """h = g |col - c0|, zones are bands of `band` rows, the row area is 2 * 2^(row % 3) * 1: all powers of two"""
    n, m = shape
    rows, cols = np.arange(n), np.arange(m)
    zone = np.repeat((rows // band + 1)[:, None], m, axis=1)
    hand = np.repeat((WEDGE_G * np.abs(cols - c0))[None, :], n, axis=0)
    return case(zone, hand, WEDGE_STAGES, dX2=2.0 * 2.0 ** (rows % 3), dY2=np.ones(n))


def wedge_closed_form(shape, band, c0):
    """(cells, area, volume, above) of wedge_case: (K, S) arrays and (K,), from one sum over the columns and one over the rows"""
    n, m = shape
    rows, cols = np.arange(n), np.arange(m)
    h = WEDGE_G * np.abs(cols - c0)
    a_row = 2.0 * 2.0 ** (rows % 3)
    K = (n - 1) // band + 1
    n_rows = np.bincount(rows // band, minlength=K)
    a_zone = np.bincount(rows // band, weights=a_row, minlength=K)
    st = np.asarray(WEDGE_STAGES)
    wet = h[None, :] <= st[:, None]                                     # (S, m)
    n_cols = wet.sum(axis=1)
    depth = np.where(wet, st[:, None] - h[None, :], 0.0).sum(axis=1)
    return (n_rows[:, None] * n_cols[None, :], a_zone[:, None] * n_cols[None, :], a_zone[:, None] * depth[None, :],
            n_rows * (m - n_cols[-1]))


def on_stage_case():
    """every cell of a column exactly on a stage: column j lies in bin j"""
    st = [0.25, 0.5, 1.0, 3.0]
    return case(np.ones((3, 4), np.int32), np.repeat(np.asarray(st)[None, :], 3, axis=0), st)


def zeros_case():
    """+0.0 and -0.0 with stages[0] = 0: both in bin 0"""
    hand = np.zeros((4, 6))
    hand[:, ::2] = -0.0
    return case(np.ones((4, 6), np.int32), hand, [0.0, 1.0])


def negative_case():
    """h = -2 below stages[0] = -1 (bin 0), h = -0.5 in bin 1, h = 0.5 in bin 2"""
    hand = np.empty((3, 6))
    hand[:, :2], hand[:, 2:4], hand[:, 4:] = -2.0, -0.5, 0.5
    return case(np.ones((3, 6), np.int32), hand, [-1.0, 0.0, 1.0])


def skipped_case():
    """NaN, +inf and a value above the top; zones 0 and -1 are not counted anywhere; a non-finite slope counts as 0"""
    zone = np.array([[1, 1, 1, 1, 2, 2, 0, -1],
                     [1, 1, 2, 2, 2, 2, 0, -1],
                     [0, -1, 0, -7, 0, 0, -1, 0]], np.int32)            # (a tile has three rows at least)
    hand = np.array([[0.5, np.nan, np.inf, 4.0, 0.5, 1.0, 0.5, 0.5],
                     [1.0, 0.25, np.nan, np.nan, 2.5, 0.5, np.nan, np.inf],
                     [0.5, 1.0, np.nan, 0.25, np.inf, 2.0, 0.5, -3.0]])
    mag = np.full(zone.shape, 0.75)
    mag[1, 0], mag[1, 1] = np.nan, np.inf
    return case(zone, hand, [0.5, 1.0, 2.0], mag=mag, K=3)              # (zone 3 exists and is empty)


def single_stage_case():
    hand = np.repeat(np.array([0.0, 0.5, 1.0, 1.5, 2.0])[None, :], 4, axis=0)
    return case(np.repeat(np.array([1, 2, 1, 2])[:, None], 5, axis=1), hand, [1.0])


def designed_cases():
    return [('uniform', uniform_case()), ('wedge', wedge_case((12, 23), 5, 9)), ('on_stage', on_stage_case()), ('zeros', zeros_case()),
            ('negative', negative_case()), ('skipped', skipped_case()), ('single_stage', single_stage_case())]


def random_case(shape, K, S, seed, nan_share=0.10, per_row=False):
    """random HAND in [-1, 30) with `nan_share` NaN and some +inf, zones -1 .. K, a random slope with flats (-1) and NaN"""
    rng = np.random.default_rng(seed)
    n, m = shape
    zone = rng.integers(-1, K + 1, shape).astype(np.int32)
    hand = rng.uniform(-1.0, 30.0, shape)
    hand[rng.random(shape) < nan_share] = np.nan
    hand[rng.random(shape) < 0.01] = np.inf
    stages = np.sort(rng.uniform(0.0, 25.0, S))
    hand[rng.random(shape) < 0.02] = stages[rng.integers(0, S)]         # cells exactly on a stage
    mag = rng.uniform(0.0, 2.0, shape)
    mag[rng.random(shape) < 0.05] = -1.0
    mag[rng.random(shape) < 0.02] = np.nan
    dX2 = rng.uniform(20.0, 40.0, n) if per_row else np.full(n, 30.0)
    dY2 = rng.uniform(20.0, 40.0, n) if per_row else np.full(n, 30.0)
    return case(zone, hand, stages, dX2=dX2, dY2=dY2, mag=mag, K=K)


def ref(c):
    return H.hand_table_ref(c['zone'], c['hand'], c['stages'], c['dX2'], c['dY2'], c['mag'], c['K'])


def table_of(c, length=None, slope=None, manning_n=0.05):
    ints, skipped, quanta = ref(c)
    K = c['K']
    return H.hydraulic_table(ints, quanta, c['stages'], np.ones(K) if length is None else length, np.ones(K) if slope is None else slope,
                             manning_n), ints, skipped, quanta


def assert_conserved(c, ints, skipped):
    z = c['zone'].ravel()
    want = np.bincount(z[z >= 1], minlength=c['K'] + 1)[1:]
    assert np.array_equal(ints[:, :, H.CELLS].sum(axis=1) + skipped.sum(axis=1), want)


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def test_uniform_plane():
    c = uniform_case()
    tab, ints, skipped, quanta = table_of(c)
    assert ints.shape == (1, 3, 4) and ints.dtype == np.int64 and skipped.tolist() == [[0, 0]]
    assert ints[0, :, H.CELLS].tolist() == [0, 60, 0]
    shift, q = fixed_point(60, 8.0)
    assert quanta == (q, fixed_point(60, 4.0)[1], fixed_point(60, 10.0)[1]) and q == 2.0 ** -36
    assert ints[0, 1].tolist() == [60, 60 * 8 * 2 ** 36, 60 * 4 * 2 ** 37, 60 * 10 * 2 ** 36]
    assert tab['cells'].tolist() == [[0, 60, 60]]
    assert tab['area'].tolist() == [[0.0, 480.0, 480.0]]
    assert tab['volume'].tolist() == [[0.0, 0.0, 240.0]]
    assert tab['bed_area'].tolist() == [[0.0, 600.0, 600.0]]
    assert_conserved(c, ints, skipped)


@pytest.mark.parametrize('shape,band,c0', [((12, 23), 5, 9), ((64, 64), 16, 0), ((33, 40), 7, 39)])
def test_wedge(shape, band, c0):
    c = wedge_case(shape, band, c0)
    tab, ints, skipped, _ = table_of(c)
    cells, area, volume, above = wedge_closed_form(shape, band, c0)
    assert np.array_equal(tab['cells'], cells)
    assert np.array_equal(tab['area'], area)
    assert np.array_equal(tab['volume'], volume)
    assert np.array_equal(tab['bed_area'], 1.25 * area)
    assert np.array_equal(skipped[:, 1], above) and not skipped[:, 0].any()
    assert_conserved(c, ints, skipped)


def test_cells_on_a_stage_lie_in_its_bin():
    c = on_stage_case()
    ints, skipped, _ = ref(c)
    assert ints[0, :, H.CELLS].tolist() == [3, 3, 3, 3] and not skipped.any()
    tab = table_of(c)[0]
    # a cell on the stage is wet at that stage, with depth 0: area counts it, volume does not
    assert tab['area'].tolist() == [[24.0, 48.0, 72.0, 96.0]]
    assert tab['volume'].tolist() == [[0.0, 8 * 3 * 0.25, 8 * 3 * (0.75 + 0.5), 8 * 3 * (2.75 + 2.5 + 2.0)]]


def test_signed_zeros():
    c = zeros_case()
    tab, ints, skipped, quanta = table_of(c)
    assert ints[0, :, H.CELLS].tolist() == [24, 0] and ints[0, 0, H.MOMENT] == 0 and quanta[1] == fixed_point(24, 0.0)[1]
    assert tab['volume'].tolist() == [[0.0, 192.0]] and tab['area'].tolist() == [[192.0, 192.0]]
    swapped = dict(c, stages=np.array([-0.0, 1.0]))
    assert all(np.array_equal(a, b) for a, b in zip(ref(swapped)[:2], (ints, skipped)))


def test_negative_hand():
    c = negative_case()
    tab, ints, skipped, _ = table_of(c)
    assert ints[0, :, H.CELLS].tolist() == [6, 6, 6] and not skipped.any()
    assert ints[0, 0, H.MOMENT] < 0
    assert tab['area'].tolist() == [[48.0, 96.0, 144.0]]
    assert tab['volume'].tolist() == [[48.0 * 1.0, 48.0 * 2.0 + 48.0 * 0.5, 48.0 * 3.0 + 48.0 * 1.5 + 48.0 * 0.5]]


def test_nan_inf_and_zones_below_one():
    c = skipped_case()
    tab, ints, skipped, _ = table_of(c)
    assert skipped.tolist() == [[1, 2], [2, 1], [0, 0]]
    assert ints[:, :, H.CELLS].tolist() == [[2, 1, 0], [2, 1, 0], [0, 0, 0]]
    assert_conserved(c, ints, skipped)
    # zone 1, bin 0: (0, 0) with slope 0.75 and (1, 1) with slope inf -> 1; bin 1: (1, 0) with slope NaN -> 1
    assert tab['bed_area'][0].tolist() == [8 * 1.25 + 8.0, 8 * 1.25 + 8.0 + 8.0, 8 * 1.25 + 8.0 + 8.0]
    assert not tab['cells'][2].any() and np.isnan(tab['discharge'][2]).all()
    with pytest.raises(ValueError):
        H.hand_table_ref(c['zone'], c['hand'], c['stages'], c['dX2'], c['dY2'], c['mag'], 1)         # a zone above K
    bad = c['hand'].copy()
    bad[0, 0] = -np.inf
    with pytest.raises(ValueError):
        H.hand_table_ref(c['zone'], bad, c['stages'], c['dX2'], c['dY2'], c['mag'], 3)


def test_single_stage():
    c = single_stage_case()
    tab, ints, skipped, _ = table_of(c)
    assert ints.shape == (2, 1, 4) and ints[:, 0, H.CELLS].tolist() == [6, 6] and skipped.tolist() == [[0, 4], [0, 4]]
    assert tab['volume'].tolist() == [[2 * 8 * 1.5], [2 * 8 * 1.5]]


def test_no_zones():
    c = dict(uniform_case(), K=0, zone=np.zeros((6, 10), np.int32))
    ints, skipped, quanta = ref(c)
    assert ints.shape == (0, 3, 4) and skipped.shape == (0, 2) and quanta == tuple(fixed_point(60, 0.0)[1] for _ in range(3))
    assert H.hydraulic_table(ints, quanta, c['stages'], np.zeros(0), np.zeros(0), 0.05)['discharge'].shape == (0, 3)


def test_manning():
    c = uniform_case()
    tab = table_of(c, length=np.array([16.0]), slope=np.array([0.25]), manning_n=0.5)[0]
    # at stage 1: volume 240, bed 600, length 16: A = 15, P = 37.5, R = 0.4, Q = A R^(2/3) sqrt(S) / n
    assert tab['top_width'][0, 2] == 30.0 and tab['xs_area'][0, 2] == 15.0 and tab['wetted_perimeter'][0, 2] == 37.5
    assert tab['hydraulic_radius'][0, 2] == 0.4
    assert tab['discharge'][0, 2] == 15.0 * 0.4 ** (2.0 / 3.0) * 0.5 / 0.5
    assert np.isnan(tab['discharge'][0, 0]) and tab['discharge'][0, 1] == 0.0        # nothing wet: bed_area 0
    for length, slope in ((16.0, 0.0), (16.0, -0.1), (16.0, np.nan), (0.0, 0.25), (np.nan, 0.25)):
        t = table_of(c, length=np.array([length]), slope=np.array([slope]))[0]
        assert np.isnan(t['discharge']).all()


# ---- random planes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,K,S,seed,per_row', [((40, 50), 7, 5, 0, False), ((96, 80), 30, 32, 1, True), ((64, 64), 1, 1, 2, False)])
def test_random_planes_against_float_sums(shape, K, S, seed, per_row):
    c = random_case(shape, K, S, seed, per_row=per_row)
    ints, skipped, quanta = ref(c)
    assert_conserved(c, ints, skipped)
    n, m = shape
    a = np.repeat((c['dX2'] * c['dY2'])[:, None], m, axis=1).ravel()
    z, h, mg = c['zone'].ravel(), c['hand'].ravel(), c['mag'].ravel()
    with np.errstate(invalid='ignore'):
        counted = (z >= 1) & ~np.isnan(h) & ~(h > c['stages'][-1])
        slope = np.where(np.isfinite(mg), np.sqrt(1.0 + mg * mg), 1.0)
    key = (z[counted] - 1) * S + np.searchsorted(c['stages'], h[counted], 'left')
    cells = np.bincount(key, minlength=K * S).reshape(K, S)
    assert np.array_equal(ints[:, :, H.CELLS], cells) and cells.sum() > 0
    for col, p, q in ((H.AREA, a, quanta[0]), (H.MOMENT, a * h, quanta[1]), (H.BED, a * slope, quanta[2])):
        plain = np.bincount(key, weights=p[counted], minlength=K * S).reshape(K, S)
        err = np.abs(ints[:, :, col] * q - plain)
        # the fixed point is within cells * q / 2 of the exact sum; numpy's float sum of `cells` terms is within cells * ulp(sum |p|)
        # of it (some 2^-11 of the first term at most: the quantum is 2^-40 of the largest p, an ulp 2^-52 of the sum)
        bound = cells * q / 2 + cells * np.spacing(np.bincount(key, weights=np.abs(p[counted]), minlength=K * S).reshape(K, S))
        assert (err <= bound).all(), (col, float((err - bound).max()))
