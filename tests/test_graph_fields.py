"""tests/graph_fields.py held to its own claims, on the CPU: the numpy restatement of the reference's section / proportion lines
and the oracle agree bit for bit on directions no golden shows either of them; every field is acyclic; and the fields together
reach what they are named for -- every class of designed value, every outcome of the keep-filter per facet kind, every inlet
and corner case, both sides of every threshold.  And glibc's log against the long-double logarithm on the TWI inputs, printed:
the yardstick for what tests/test_gpu_graph_bits.py measures of the device's."""
import numpy as np
import pytest

import graph_fields as GF
from flowgraph_kit import assert_same_bits


@pytest.mark.parametrize('field', GF.graph_fields(), ids=lambda f: f.name)
def test_restatement_and_oracle_agree_to_the_bit(field):
    from oracle import oracle as O
    sec_np, prop_np = GF.section_proportion(field.direction, field.flats, field.dX, field.dY)
    sec, prop = O.section_proportion(field.direction, field.flats, field.dX, field.dY)
    assert np.array_equal(sec, sec_np), (sec != sec_np).sum()
    assert_same_bits(prop, prop_np, 'proportion, ' + field.name)
    o = GF.oracle_of(field)
    assert np.array_equal(o.section, sec) and o.proportion.tobytes() == prop.tobytes()        # calc_uca saw the planes that were set
    assert ((sec >= -1) & (sec <= 7)).all()
    assert np.array_equal(sec == -1, field.flats.astype(bool))


@pytest.mark.parametrize('field', GF.graph_fields(), ids=lambda f: f.name)
def test_every_field_is_acyclic(field):
    o = GF.oracle_of(field)
    assert o.stats[0] == 1 and o.stats[2] == 0, o.stats          # one drain_area call, no circular cells left
    assert o.stats[1] >= 2


def test_spacing_and_shapes_are_what_the_kernels_need():
    fields = GF.graph_fields()
    assert [f.shape for f in fields] == [(3, 3), (3, 300), (24, 300), (300, 5), (20, 70), (5, 7)]
    uniform = [bool((f.dX == f.dX[0]).all() and (f.dY == f.dY[0]).all()) for f in fields]
    assert uniform.count(True) >= 1 and uniform.count(False) >= 2
    tall = GF.tall_field()
    th = tall.theta
    assert th[0] == th[1] and th[-1] == th[-2] and np.unique(th).size == tall.shape[0] - 2      # the clamp, and a theta per row otherwise
    assert np.unique(GF.tiny_field().theta).size == 1
    for f in fields:
        d = f.direction[f.flats == 0]
        assert not (d < 0).any() and not (d > 2 * np.pi).any()                                   # NaN apart, within the stencil's range
        assert ((f.mag == -1) == (f.flats == 1)).all() and (f.direction[f.flats == 1] == -1).all()


def _counts():
    out = []
    for f in GF.graph_fields():
        o = GF.oracle_of(f)
        out.append(GF.graph_stats(f, o.section, o.proportion, o.A))
    return out


def test_the_fields_cover_what_they_are_named_for():
    per_field = _counts()
    total = GF.merge_counts(per_field)
    for k in sorted(total):
        print('%-60s %s' % (k, ' '.join('%6d' % c.get(k, 0) for c in per_field)))
    missing = [k for k, v in total.items() if v <= 0]
    assert not missing, missing
    # the block field alone reaches every section, both sides of every comparison and every keep-filter outcome
    block = per_field[[f.name for f in GF.graph_fields()].index(GF.block_field().name)]
    for k, v in block.items():
        if k.startswith(('section', 'q', 'cardinal', 'diagonal', 'out-degree', 'proportion', '0 <', 'left', 'right', 'top', 'bottom')):
            assert v > 0, k
    # every class of designed value is on some cell (a later builder may take a cell over: counted on what is left)
    placed = set().union(*[f.labels() for f in GF.graph_fields()])
    assert sorted(placed) == GF.expected_labels()
    for f in (GF.strip_field(), GF.block_field()):
        assert sorted(f.labels()) == GF.expected_labels(), f.name
    # what the builders placed is what the oracle finds there
    tall = GF.tall_field()
    o = GF.oracle_of(tall)
    i, j = tall.exact_tol_cell
    indptr, _, data = o.A
    c = i * tall.shape[1] + j
    assert indptr[c + 1] - indptr[c] == 1 and data[indptr[c]] == 1e-2 and o.section[i, j] == 1
    assert not o.edge_todo[i, j]                                   # outsum > TOL is false at equality


def test_inlet_and_corner_masks_follow_the_designed_cases():
    for f in GF.graph_fields():
        o = GF.oracle_of(f)
        n, m = f.shape
        for case in GF.CORNER_CASES:
            for ci, cj in f.notes.get('corner_' + case, []):
                assert bool(o.edge_todo[ci, cj]) == GF.CORNER_TODO[case], (f.name, case)
        for side in ('left', 'right', 'top', 'bottom'):
            cells = f.notes.get('inlet_' + side, [])
            todo = [bool(o.edge_todo[c]) for c in cells]
            assert todo == [False, False, True, True][:len(todo)], (f.name, side, todo)      # 0.0099 twice, then 0.0101 twice


def test_drained_pits_keep_the_section_of_the_mask_before_the_search():
    f = GF.pit_field()
    o = GF.oracle_of(f)
    pits = tuple(np.array(GF.PITS).T)
    assert o.pit_i.size >= len(GF.PITS) and not o.flats[pits].any() and (o.mag[pits] >= 0).all()     # drained: mask and slope patched
    assert (o.section[pits] == -1).all() and np.isnan(o.proportion[pits]).all()
    assert set(np.unique(o.pit_i).tolist()) == set(int(i * f.shape[1] + j) for i, j in GF.PITS)


def test_twi_inputs_reach_what_they_are_named_for():
    cases = GF.twi_cases(large=False)
    q = np.concatenate([c.quotient().ravel() for c in cases])
    one = np.float64(1.0)
    for k in (-2, -1, 0, 1, 2):
        assert (q == GF._steps(one, k)).any(), k
    for k in range(10, 53):
        assert (q == 1 + 2.0 ** -k).any() and (q == 1 - 2.0 ** -k).any(), k
    tiny = np.finfo(np.float64).tiny
    assert ((q > 0) & (q < tiny)).any() and (q > 1e307).any() and np.isposinf(q).any() and np.isnan(q).any() and (q == 0).any() and (q < 0).any()
    assert sorted(set((c.lim_twi, c.lim_uca) for c in cases if c.name.startswith('specials'))) == [(False, False), (False, True), (True, False), (True, True)]
    assert any(np.isinf(c.min_area) for c in cases)
    for c in cases:
        if c.name.startswith('specials') and np.isfinite(c.min_area):
            cap_u = c.sat * c.min_area
            for k in (-1, 0, 1):
                assert (c.uca == GF._steps(cap_u, k)).any()
                if k <= 0 or not c.lim_uca:                        # (with the limit on uca no quotient of this tile is above the cap's)
                    assert (c.quotient() == GF._steps(cap_u / c.min_slope, k)).any()
            if not c.lim_uca:
                # RESULTS one ulp below the cap, at it and one ulp above it: visible without the limit, capped with it
                from oracle import oracle as O
                cap = c.cap()
                free = O.twi(c.uca, c.mag, c.min_slope, c.min_area, c.sat, False, False)
                for j in GF.NEAR_CAP_ULPS:
                    assert (free == GF._steps(cap, j)).any(), j
                got = O.twi(c.uca, c.mag, c.min_slope, c.min_area, c.sat, c.lim_twi, False)
                if c.lim_twi:
                    near = np.abs(free - cap) <= 5 * np.spacing(cap)
                    assert np.array_equal(got[near], np.minimum(free[near], cap)) and not (got[near] > cap).any()
                    assert (got == GF._steps(cap, -1)).any() and ((got == cap) & (free == GF._steps(cap, 1))).any()
                else:
                    assert (got == GF._steps(cap, 1)).any()
            assert (c.mag == -1).any() and np.isnan(c.mag).any() and (c.mag == -c.min_slope).any()
            assert (c.uca == 0).any() and np.isnan(c.uca).any() and np.isposinf(c.uca).any()
    big = GF.large_twi_case()
    assert big.uca.size == 2100000 > 8192 * 256 and np.unique(big.uca).size == big.uca.size


def test_oracle_twi_against_the_long_double_logarithm():
    """glibc's log, for the record: correctly rounded in all but a few cells, never a full ulp off.  The bound asserted is the one
    the device is held to (tests/test_gpu_graph_bits.py)."""
    from oracle import oracle as O
    worst = 0.0
    for c in GF.twi_cases():
        ref = O.twi(c.uca, c.mag, c.min_slope, c.min_area, c.sat, c.lim_twi, c.lim_uca)
        w, measured, capped = GF.twi_check(c, ref, ref, 3.0)
        print('%-34s worst %.4f ulp over %d cells, %d capped' % (c.name, w, measured, capped))
        worst = max(worst, w)
    print('glibc log: worst %.4f ulp' % worst)
    assert worst <= 1.0
