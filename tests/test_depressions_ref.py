"""CPU tier: the host twin of the depression inventory (pydem_amd/conditioning.py: label_depressions, fill_depressions_limited)
against a plain Python flood written here, on designed fields; the component counts the definition rests on; the properties of
every depression; the filters; the limited fill."""
import numpy as np
import pytest

import depression_fields as D
import fill_fields as F

INT_COLUMNS = ('cells', 'r0', 'r1', 'c0', 'c1', 'spill_elev', 'bottom_row', 'bottom_col', 'bottom_elev', 'max_depth', 'pour_row',
               'pour_col', 'n_sills', 'open_sill')


def cases():
    d = dict(D.builders())
    d.update(F.designed())
    d['fractal96'] = lambda: F.fractal(96, 80)
    return d


_CACHE = {}


def twin(name):
    """(z, W, label, table, quanta, row_area) of a case, computed once"""
    if name not in _CACHE:
        from pydem_amd import conditioning
        z = np.asarray(cases()[name](), dtype=np.float64)
        ra = D.row_area(name, z.shape[0])
        W = conditioning.fill_depressions(z, 0.0)[0]
        label, table, quanta = conditioning.label_depressions(z, dX2dY2=ra)
        _CACHE[name] = (z, W, label, table, quanta, ra)
    return _CACHE[name]


def slow_reference(z, W, outlets=None):
    """A plain flood over W > z in raster order: label raster and one dict per depression (every exact column)."""
    n, m = z.shape
    zl, Wl = z.tolist(), W.tolist()
    raised = [[Wl[r][c] > zl[r][c] for c in range(m)] for r in range(n)]
    nan = [[zl[r][c] != zl[r][c] for c in range(m)] for r in range(n)]
    label = [[-1 if nan[r][c] else 0 for c in range(m)] for r in range(n)]
    nbrs = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]

    def is_open(r, c):
        if r in (0, n - 1) or c in (0, m - 1) or (outlets is not None and outlets[r][c]):
            return True
        return any(nan[r + dr][c + dc] for dr, dc in nbrs)

    rows = []
    for r0 in range(n):
        for c0 in range(m):
            if not raised[r0][c0] or label[r0][c0]:
                continue
            k = len(rows) + 1
            label[r0][c0] = k
            stack, cells = [(r0, c0)], []
            while stack:
                r, c = stack.pop()
                cells.append((r, c))
                for dr, dc in nbrs:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < n and 0 <= cc < m and raised[rr][cc] and not label[rr][cc]:
                        label[rr][cc] = k
                        stack.append((rr, cc))
            S = Wl[r0][c0]
            zmin = min(zl[r][c] for r, c in cells)
            bottom = min((r, c) for r, c in cells if zl[r][c] == zmin)
            sills = set()
            for r, c in cells:
                for dr, dc in nbrs:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < n and 0 <= cc < m and not raised[rr][cc] and not nan[rr][cc] and zl[rr][cc] == S:
                        sills.add((rr, cc))
            pour = min(sills)
            rows.append(dict(cells=len(cells), r0=min(r for r, _ in cells), r1=max(r for r, _ in cells),
                             c0=min(c for _, c in cells), c1=max(c for _, c in cells), spill_elev=S, bottom_row=bottom[0],
                             bottom_col=bottom[1], bottom_elev=zl[bottom[0]][bottom[1]], max_depth=S - zl[bottom[0]][bottom[1]],
                             pour_row=pour[0], pour_col=pour[1], n_sills=len(sills), open_sill=int(any(is_open(r, c) for r, c in sills)),
                             cell_list=cells))
    return np.array(label, dtype=np.int32).reshape(n, m), rows


def fixed_point_numpy(z, W, label, K, ra):
    """area and volume by the integer definition of the header, recomputed in numpy: (area, volume, quanta, sums of p)"""
    n, m = z.shape
    B = min(40, 62 - int(np.ceil(np.log2(max(n * m, 2)))))
    with np.errstate(invalid='ignore'):
        depth = np.where(W > z, W - z, 0.0)
    p_area = np.broadcast_to(ra[:, None], z.shape)
    p_vol = depth * ra[:, None]
    out = []
    for p, largest in ((p_area, ra.max()), (p_vol, depth.max() * ra.max())):
        E = int(np.frexp(largest)[1])
        q = 2.0 ** (E - B)
        ticks = np.rint(p / q).astype(np.int64)
        col = np.array([float(int(ticks[label == k].sum())) * q for k in range(1, K + 1)])
        plain = np.array([p[label == k].sum() for k in range(1, K + 1)])
        out.append((col, q, plain))
    return out


@pytest.mark.parametrize('name', sorted(cases()))
def test_host_twin_against_a_plain_flood(name):
    z, W, label, table, quanta, ra = twin(name)
    ref_label, rows = slow_reference(z, W)
    assert label.dtype == np.int32 and np.array_equal(label, ref_label)
    assert len(table) == len(rows)
    for col in INT_COLUMNS:
        want = np.array([row[col] for row in rows], dtype=table.dtype[col])
        assert np.array_equal(table[col], want), col
    K = len(rows)
    (area, q_a, sum_a), (volume, q_v, sum_v) = fixed_point_numpy(z, W, ref_label, K, ra)
    assert quanta == (q_a, q_v)
    assert np.array_equal(table['area'], area) and np.array_equal(table['volume'], volume)
    cells = table['cells'].astype(np.float64)
    # the header's bound, plus the rounding of the float sum it is compared with
    assert (np.abs(table['area'] - sum_a) <= cells * q_a / 2 + cells * 2.0 ** -52 * sum_a).all()
    assert (np.abs(table['volume'] - sum_v) <= cells * q_v / 2 + cells * 2.0 ** -52 * sum_v).all()
    assert np.array_equal(table['mean_depth'], table['volume'] / table['area'])


def test_component_counts():
    from scipy import ndimage
    assert len(twin('fractal96')[3]) == 66
    assert len(twin('terraces')[3]) == 36
    t = twin('serpentine')[3]
    assert len(t) == 1 and t['cells'][0] == 4656
    assert len(twin('checkerboard')[3]) == 31 * 31
    assert len(twin('diagonal_chain')[3]) == 1 and twin('diagonal_chain')[3]['cells'][0] == len(D.diagonal_chain_cells())
    assert len(twin('ring_lake')[3]) == 2 and len(twin('comb')[3]) == 1 and len(twin('two_levels')[3]) == 2
    for name in ('plateau', 'all_nan'):
        assert len(twin(name)[3]) == 0
    from pydem_amd import conditioning
    label, table, _ = conditioning.label_depressions(np.array([[5.0, 1.0, 5.0, 0.0, 5.0, 2.0, 5.0]]))
    assert label.shape == (1, 7) and len(table) == 0 and not label.any()
    # the diagonals are in
    z, W = twin('fractal96')[:2]
    assert ndimage.label(W > z)[1] > 66
    assert ndimage.label(twin('diagonal_chain')[1] > twin('diagonal_chain')[0])[1] == len(D.diagonal_chain_cells())


def test_designed_fields_are_what_they_claim():
    t = twin('ring_lake')[3]
    assert list(t['spill_elev']) == [100.0, 110.0]
    assert t['r0'][0] < t['r0'][1] and t['r1'][1] < t['r1'][0] and t['c0'][0] < t['c0'][1] and t['c1'][1] < t['c1'][0]
    t = twin('two_levels')[3]
    assert list(t['spill_elev']) == [80.0, 90.0] and list(t['n_sills']) == [1, 1]
    assert (t['pour_row'][0], t['pour_col'][0], t['pour_row'][1], t['pour_col'][1]) == (20, 9, 20, 51)
    assert list(t['open_sill']) == [0, 0]
    t = twin('lake_nan_hole')[3]
    assert len(t) == 1 and t['open_sill'][0] == 1 and t['spill_elev'][0] == 70.0 and t['n_sills'][0] == 16
    t = twin('diagonal_chain')[3]
    assert (t['pour_row'][0], t['pour_col'][0], t['spill_elev'][0], t['n_sills'][0]) == (9, 10, 60.0, 1)
    t = twin('limits')[3]
    assert list(t['max_depth']) == [40.0, 10.0]              # (the deep cone's first cell comes first in raster order)
    assert (t['bottom_row'][0], t['bottom_col'][0]) == D.LIMITS_DEEP_BOTTOM
    assert (t['bottom_row'][1], t['bottom_col'][1]) == D.LIMITS_SHALLOW_BOTTOM
    t = twin('varying_spacing')[3]
    ra = twin('varying_spacing')[5]
    assert len(t) == 1 and ra.min() < 0.9 * ra.max()


@pytest.mark.parametrize('name', sorted(cases()))
def test_properties_of_every_depression(name):
    z, W, label, table, _, _ = twin(name)
    with np.errstate(invalid='ignore'):
        raised = W > z
    depth = W - z
    assert np.array_equal(label > 0, raised) and np.array_equal(label == -1, np.isnan(z))
    n, m = z.shape
    first = -1
    for k, row in enumerate(table, start=1):
        inside = label == k
        rr, cc = np.nonzero(inside)
        assert rr.size == row['cells']
        assert rr[0] * m + cc[0] > first                        # numbered by the first cell
        first = rr[0] * m + cc[0]
        assert (W[inside] == row['spill_elev']).all()           # one level
        pr, pc = row['pour_row'], row['pour_col']
        assert not raised[pr, pc] and z[pr, pc] == row['spill_elev'] == W[pr, pc]
        assert inside[max(pr - 1, 0):pr + 2, max(pc - 1, 0):pc + 2].any()
        assert inside[row['bottom_row'], row['bottom_col']] and row['bottom_elev'] == z[row['bottom_row'], row['bottom_col']]
        assert row['bottom_elev'] == z[inside].min()
        assert row['max_depth'] == depth[inside].max()
        assert (row['r0'], row['r1'], row['c0'], row['c1']) == (rr.min(), rr.max(), cc.min(), cc.max())


def test_filters_drop_and_renumber():
    from pydem_amd import conditioning
    z, W, label, table, _, ra = twin('fractal96')
    for kw in (dict(min_depth=float(np.median(table['max_depth']))), dict(min_cells=4), dict(min_volume=float(np.median(table['volume']))),
               dict(min_depth=1.0, min_cells=3, min_volume=float(np.percentile(table['volume'], 30)))):
        keep = ((table['max_depth'] >= kw.get('min_depth', 0.0)) & (table['cells'] >= kw.get('min_cells', 1)) &
                (table['volume'] >= kw.get('min_volume', 0.0)))
        assert 0 < keep.sum() < len(table)
        lab2, tab2, _ = conditioning.label_depressions(z, dX2dY2=ra, **kw)
        assert np.array_equal(tab2, table[keep])                # the same rows in the same order
        lut = np.zeros(len(table) + 1, np.int32)
        lut[1:][keep] = np.arange(1, keep.sum() + 1)
        assert np.array_equal(lab2, np.where(label > 0, lut[np.maximum(label, 0)], label))
        assert (lab2[np.isin(label, 1 + np.flatnonzero(~keep))] == 0).all()


def test_outlet_at_the_bottom_removes_the_lake():
    from pydem_amd import conditioning
    z = D.two_levels()
    out = np.zeros(z.shape, bool)
    out[15, 40] = True                                          # in the right lake's flat bed: the whole bed drains
    label, table, _ = conditioning.label_depressions(z, out)
    assert len(table) == 1 and table['spill_elev'][0] == 80.0 and not label[:, 31:].any()


def test_limited_fill():
    from pydem_amd import conditioning
    z = D.limits()
    z0 = z.copy()
    W, depth, eps, kept = conditioning.fill_depressions_limited(z, max_depth=20.0)
    assert kept.tolist() == [list(D.LIMITS_DEEP_BOTTOM)]
    r, c = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    shallow = np.hypot(r - 32, c - 25) <= 12
    assert (W[shallow] >= 100.0).all() and (W[shallow] < 100.001).all()                               # filled to the plateau (+ epsilon steps)
    assert W[D.LIMITS_PIT] > z[D.LIMITS_PIT] and W[D.LIMITS_PIT] < 79.0                                  # the inner pit: to its own sill
    assert W[D.LIMITS_DEEP_BOTTOM] == 60.0
    deep = (np.hypot(r - 32, c - 70) <= 20)
    deep[D.LIMITS_PIT] = False
    assert np.allclose(W[deep], z[deep], atol=1e-3, rtol=0) and (W[deep] >= z[deep]).all()              # (epsilon steps only)
    assert depth.tobytes() == (W - z).tobytes()
    # a limit nothing exceeds: the plain fill
    W2, depth2, eps2, kept2 = conditioning.fill_depressions_limited(z, max_depth=50.0)
    ref = conditioning.fill_depressions(z, None)
    assert W2.tobytes() == ref[0].tobytes() and depth2.tobytes() == ref[1].tobytes() and eps2 == ref[2] and kept2.shape == (0, 2)
    # no limit at all
    W3 = conditioning.fill_depressions_limited(z)
    assert W3[0].tobytes() == ref[0].tobytes() and W3[3].shape == (0, 2)
    # max_depth=2 needs two rounds: both cones first, then the pit inside the deep one
    W4, _, _, kept4 = conditioning.fill_depressions_limited(z, max_depth=2.0, epsilon=0.0)
    assert sorted(kept4.tolist()) == sorted([list(D.LIMITS_SHALLOW_BOTTOM), list(D.LIMITS_DEEP_BOTTOM), list(D.LIMITS_PIT)])
    assert kept4.tolist()[2] == list(D.LIMITS_PIT) and W4.tobytes() == z.tobytes()
    with pytest.raises(RuntimeError, match='max_rounds'):
        conditioning.fill_depressions_limited(z, max_depth=2.0, max_rounds=1)
    assert z.tobytes() == z0.tobytes()
    # the other limits
    assert conditioning.fill_depressions_limited(z, max_cells=600)[3].tolist() == [list(D.LIMITS_DEEP_BOTTOM)]
    t = conditioning.label_depressions(z)[1]
    assert conditioning.fill_depressions_limited(z, max_volume=float(t['volume'].mean()))[3].tolist() == [list(D.LIMITS_DEEP_BOTTOM)]
