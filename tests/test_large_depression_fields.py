"""CPU tier: the exact references of tests/large_depression_fields.py against the host twins (pydem_amd/conditioning.py:
fill_depressions, label_depressions) at a size the host flood follows -- the composed mosaic against the flood of the whole tile,
the great lake's closed form against both twins.  Bytes and array_equal throughout."""
import math

import numpy as np
import pytest

import large_depression_fields as L
from depression_checks import same

SMALL = (330, 400)          # three shelves of the cycle
LAKE = (70, 90)

_WHOLE = {}


def whole_fill(eps):
    """the host flood of the whole small mosaic, once per epsilon"""
    if eps not in _WHOLE:
        from pydem_amd import conditioning
        _WHOLE[eps] = conditioning.fill_depressions(L.mosaic(*SMALL).z, eps)
    return _WHOLE[eps]


def test_the_small_mosaic_is_the_one_asked_for():
    mo = L.mosaic(*SMALL)
    assert len(mo.placements) >= 12 and len({r for _, r, _ in mo.placements}) == 3
    assert len({(r % 32, c % 32) for _, r, c in mo.placements}) >= 6
    # a patch over a multiple of 32 in both directions, away from the tile's origin
    assert any(r > 0 and c > 0 and (r - 1) // 32 != (r + L.patch(nm).shape[0] - 1) // 32 and r % 32 != 0
               and (c - 1) // 32 != (c + L.patch(nm).shape[1] - 1) // 32 and c % 32 != 0 for nm, r, c in mo.placements)
    # one no-data row or column between neighbours, no data in the rest
    covered = np.zeros(mo.z.shape, bool)
    for nm, r, c in mo.placements:
        h, w = L.patch(nm).shape
        assert not covered[max(r - 1, 0):r + h + 1, max(c - 1, 0):c + w + 1].any()
        covered[r:r + h, c:c + w] = True
        assert mo.z[r:r + h, c:c + w].tobytes() == L.patch(nm).tobytes()
    assert np.isnan(mo.z[~covered]).all()


@pytest.mark.parametrize('eps', [0.0, None])
def test_composed_fill_is_the_flood_of_the_whole_tile(eps):
    mo = L.mosaic(*SMALL)
    W, depth, used = whole_fill(eps)
    assert used == mo.epsilon(eps)
    if eps is None:
        from pydem_amd import conditioning
        own = {conditioning.fill_depressions_epsilon(L.patch(nm), None) for nm, _, _ in mo.placements}
        assert used == max(own) and len(own) > 1        # the tile's epsilon is not every patch's own
    assert mo.fill(eps).tobytes() == W.tobytes()
    with np.errstate(invalid='ignore'):
        assert (W > mo.z).sum() >= 1000


@pytest.mark.parametrize('varying', [False, True])
def test_composed_inventory_is_the_inventory_of_the_whole_tile(varying):
    from pydem_amd import conditioning
    mo = L.mosaic(*SMALL)
    n = SMALL[0]
    ra = L.row_area(n) if varying else np.full(n, 900.0)
    want = conditioning.label_depressions(mo.z, dX2dY2=ra)
    got = mo.inventory(ra)
    assert len(want[1]) >= 1000 and mo.labels()[1] == len(want[1])
    same(dict(label=got[0], table=got[1]), want, dict(quanta=got[2]))
    # filtered the same way
    kw = dict(min_depth=2.0, min_cells=2)
    want = conditioning.label_depressions(mo.z, dX2dY2=ra, **kw)
    assert 0 < len(want[1]) < len(got[1])
    same(dict(zip(('label', 'table'), L.filtered(got, **kw)[:2])), want)


def test_great_lake_closed_form_is_what_the_host_twins_give():
    from pydem_amd import conditioning
    lake = L.great_lake(*LAKE)
    n, m = LAKE
    ra = L.row_area(n)
    W, depth, _ = conditioning.fill_depressions(lake.z, 0.0)
    assert lake.W.tobytes() == W.tobytes()
    want = conditioning.label_depressions(lake.z, dX2dY2=ra)
    got = lake.inventory(ra)
    same(dict(label=got[0], table=got[1]), want, dict(quanta=got[2]))
    t = got[1]
    assert len(t) == 1 and t['cells'][0] == (n - 2) * (m - 2) and (t['pour_row'][0], t['pour_col'][0]) == lake.sill
    assert len(set(ra.tolist())) == n                   # every row its own area
    # the contract of the fixed-point sums
    for col, terms, q in zip(('area', 'volume'), lake.terms(ra), got[2]):
        assert abs(t[col][0] - math.fsum(terms.tolist())) <= lake.cells * q / 2
