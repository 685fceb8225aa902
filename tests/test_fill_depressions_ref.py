"""CPU tier: the host priority flood (pydem_amd/conditioning.py: fill_depressions), the twin the device fill is compared with,
against a deliberately different algorithm -- a whole-grid Jacobi iteration downward from +inf -- bit for bit, on the designed
surfaces of tests/fill_fields.py, and the properties the contract of pydem_fill_depressions (include/pydem_hip.h) states."""
import numpy as np
import pytest

import fill_fields as F

EPS = (0.0, 1e-6, 2.0 ** -20)


def open_cells(z, outlets=None):
    nan = np.isnan(z)
    op = np.zeros(z.shape, bool)
    op[0, :] = op[-1, :] = True
    op[:, 0] = op[:, -1] = True
    p = np.pad(nan, 1, constant_values=False)
    n, m = z.shape
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            op |= p[dr:dr + n, dc:dc + m]
    if outlets is not None:
        op |= np.asarray(outlets, bool)
    return op & ~nan


def neighbour_min(W):
    """min over the 8 neighbours; NaN cells and the outside count as +inf"""
    n, m = W.shape
    p = np.pad(np.where(np.isnan(W), np.inf, W), 1, constant_values=np.inf)
    lo = np.full(W.shape, np.inf)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if dr == 1 and dc == 1:
                continue
            lo = np.minimum(lo, p[dr:dr + n, dc:dc + m])
    return lo


def fill_depressions_ref(z, eps, outlets=None):
    """Jacobi: every cell from the previous iterate at once, from +inf, until nothing changes."""
    z = np.asarray(z, np.float64)
    nan = np.isnan(z)
    op = open_cells(z, outlets)
    W = np.where(nan, np.nan, np.inf)
    W[op] = z[op]
    free = ~op & ~nan
    for _ in range(4 * z.size + 4):
        s = neighbour_min(W) + eps
        new = np.where(s > z, s, z)
        upd = free & (new < W)
        if not upd.any():
            return W
        W = np.where(upd, new, W)
    raise AssertionError("the Jacobi reference did not converge")


@pytest.fixture(scope='module')
def fields():
    d = {nm: b() for nm, b in F.designed().items()}
    d['fractal96'] = F.fractal(96, 80)
    return d


@pytest.fixture(scope='module')
def filled(fields):
    from pydem_amd import conditioning
    return {(nm, eps): conditioning.fill_depressions(z, eps) for nm, z in fields.items() for eps in EPS}


NAMES = sorted(F.designed()) + ['fractal96']


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('eps', EPS)
def test_heap_flood_equals_jacobi_bit_for_bit(fields, filled, name, eps):
    z = fields[name]
    W, depth, used = filled[(name, eps)]
    ref = fill_depressions_ref(z, eps)
    assert used == eps
    assert W.dtype == np.float64 and W.tobytes() == ref.tobytes()
    assert depth.tobytes() == (ref - z).tobytes()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('eps', EPS)
def test_properties(fields, filled, name, eps):
    z = fields[name]
    W, depth, _ = filled[(name, eps)]
    nan = np.isnan(z)
    op = open_cells(z)
    assert np.array_equal(np.isnan(W), nan)
    assert (W[~nan] >= z[~nan]).all()
    assert W[op].tobytes() == z[op].tobytes()
    free = ~op & ~nan
    if eps > 0:
        assert (neighbour_min(W)[free] < W[free]).all()       # no interior pit or flat is left
    else:
        assert np.isin(W[~nan], z[~nan]).all()                # the classic fill invents no value


@pytest.mark.parametrize('name', ['bowl', 'nested', 'serpentine', 'negative_zero', 'fractal96'])
@pytest.mark.parametrize('eps', EPS)
def test_idempotent(filled, name, eps):
    from pydem_amd import conditioning
    W, _, _ = filled[(name, eps)]
    W2, depth2, _ = conditioning.fill_depressions(W, eps)
    assert W2.tobytes() == W.tobytes()
    assert not (depth2 > 0).any()


def test_fractal_is_a_real_input(filled):
    _, depth, _ = filled[('fractal96', 0.0)]
    assert int((depth > 0).sum()) == 737


def test_corner_spill_fills_to_the_diagonal_sill(filled):
    for k in range(4):
        W, _, _ = filled[('corner_spill%d' % k, 0.0)]
        assert set(np.unique(W[F.corner_spill_basin(k)])) == {60.0}


def test_outlet_at_the_bottom_leaves_the_bowl_unfilled(fields):
    from pydem_amd import conditioning
    z = fields['bowl']
    out = np.zeros(z.shape, bool)
    out[F.BOWL_BOTTOM] = True
    for eps in (0.0, 2.0 ** -20):
        W, depth, _ = conditioning.fill_depressions(z, eps, out)
        assert W.tobytes() == fill_depressions_ref(z, eps, out).tobytes()
        r, c = np.mgrid[0:z.shape[0], 0:z.shape[1]]
        inside = (r - F.BOWL_BOTTOM[0]) ** 2 + (c - F.BOWL_BOTTOM[1]) ** 2 <= F.BOWL_RADIUS ** 2
        assert W[F.BOWL_BOTTOM] == z[F.BOWL_BOTTOM]
        if eps == 0:
            assert W[inside].tobytes() == z[inside].tobytes()
        else:
            assert (depth[inside] <= 32 * eps).all()          # (only the gradient toward the outlet, never the lake)
    W, depth, _ = conditioning.fill_depressions(z, 0.0)
    assert depth[F.BOWL_BOTTOM] == 24.0


def test_plateau(fields, filled):
    z = fields['plateau']
    W, depth, _ = filled[('plateau', 0.0)]
    assert W.tobytes() == z.tobytes() and not depth.any()
    W, _, _ = filled[('plateau', 2.0 ** -20)]
    assert W.tobytes() == fill_depressions_ref(z, 2.0 ** -20).tobytes()
    r, c = np.mgrid[0:40, 0:70]
    steps = np.minimum(np.minimum(r, 39 - r), np.minimum(c, 69 - c))
    assert np.array_equal(W, 123.0 + steps * 2.0 ** -20)      # eps per step from the border, each sum exact


def test_automatic_epsilon(fields):
    from pydem_amd import conditioning
    z = fields['fractal96']
    assert 512 < z.max() < 1001
    W, _, used = conditioning.fill_depressions(z)
    assert used == 2.0 ** -32 * 1024
    assert W.tobytes() == fill_depressions_ref(z, used).tobytes()
    assert conditioning.fill_depressions_epsilon(np.full((4, 4), 1024.0), None) == 2.0 ** -22      # a power of two is its own bound
    assert conditioning.fill_depressions_epsilon(np.full((4, 4), -1025.0), None) == 2.0 ** -21
    assert conditioning.fill_depressions_epsilon(np.zeros((4, 4)), None) == 2.0 ** -32
    assert conditioning.fill_depressions_epsilon(np.full((4, 4), np.nan), None) == 2.0 ** -32


def test_masked_and_integer_input(fields):
    from pydem_amd import conditioning
    t = F.terraces()
    W, _, _ = conditioning.fill_depressions(t, 0.0)
    assert W.tobytes() == fill_depressions_ref(t.astype(np.float64), 0.0).tobytes()
    z = fields['bowl']
    hole = np.isnan(fields['bowl_nan_hole'])
    W, _, _ = conditioning.fill_depressions(np.ma.masked_array(z, mask=hole), 0.0)
    assert W.tobytes() == fill_depressions_ref(fields['bowl_nan_hole'], 0.0).tobytes()
    thin = np.array([[5.0, 1.0, 7.0, 0.0, 3.0, 9.0, 2.0]])
    W, depth, _ = conditioning.fill_depressions(thin, 1e-6)
    assert W.tobytes() == thin.tobytes() and not depth.any()   # every cell of a one-row tile is on the border


@pytest.mark.parametrize('eps', [-1.0, -1e-300, float('nan'), float('inf'), 'x'])
def test_bad_epsilon_is_a_value_error(fields, eps):
    from pydem_amd import conditioning
    with pytest.raises(ValueError):
        conditioning.fill_depressions(fields['bowl'], eps)


def test_ineffective_epsilon_and_infinite_cells_are_refused(fields):
    from pydem_amd import conditioning
    z = fields['bowl']
    with pytest.raises(ValueError):
        conditioning.fill_depressions(z, 2.0 ** -45)          # 550 + 2^-45 == 550
    conditioning.fill_depressions(z, 2.0 ** -43)
    bad = z.copy()
    bad[3, 3] = np.inf
    with pytest.raises(ValueError):
        conditioning.fill_depressions(bad, 0.0)
    bad[3, 3] = -np.inf
    with pytest.raises(ValueError):
        conditioning.fill_depressions(bad, 0.0)
    with pytest.raises(ValueError):
        conditioning.fill_depressions(z, 0.0, np.zeros((3, 3), bool))
    with pytest.raises(ValueError):
        conditioning.fill_depressions(z[0], 0.0)
