"""The graph stage (csrc/uca.hip: k_section_proportion with keep_edge of csrc/uca_graph.h, k_graph_inmask, k_corner_todo) and k_twi
held to the oracle on the designed inputs of tests/graph_fields.py.  The direction plane is SET on both sides (mag, direction,
flats assigned, then calc_uca / build_graph), so the device and the oracle see the same bits and nothing here has a tolerance
except what the sweep re-associates and what a logarithm is allowed.

The bars, for every field, through calc_uca(), through build_graph() on a fresh processor, and once more in a child process
whose device memory is poisoned at hand-out (PYDEM_MEM_POISON=0xA5):
  section, edge_todo, edge_done   equal to the oracle's;
  proportion                      the oracle's bits, NaN pattern included: one subtraction and one correctly rounded division in the
                                  reference's operand order;
  graph words                     out flags and in-mask describe exactly the oracle's CSC edge set, each flag paired with the share
                                  (proportion / 1 - proportion of the device's plane, formed by the test) the oracle gives that
                                  target; a pit edge's weight, which is the pit search's, within RTOL; the facet field is
                                  section & 7; build_graph() leaves the same static bits as calc_uca();
  uca                             within test_gpu_parity's RTOL / ATOL (the sweep adds in another order; the 1 - proportion it
                                  forms on the device is seen only here).

TWI (assign uca and mag, set the options, calc_twi()): the NaN / -inf / +inf pattern is the oracle's; cells beyond the cap carry
the oracle's bits (the cap is a host log in both); every other cell is measured in ulps of np.log of the float64 quotient taken
in np.longdouble -- the quotient itself is one correctly rounded division and therefore identical.  The comparison `t > twi_cap`
itself has no tolerance: the capped plane is min(the device's own uncapped plane, cap) bit for bit, on results placed 4 .. 1 ulp
below the cap, at it and 1 .. 4 ulp above it.

The bound on the logarithm, LOG_ULPS = 3: the ROCm installation this was written against states no accuracy for the device
library's fp64 log (no statement in the device-library documentation or in the HIP / clang headers shipped with it), so the bound
is the 3 ulp that the OpenCL C specification (section 7.4, "Relative error as ULPs", double precision: log <= 3 ulp) allows a
conforming double-precision log, which is the contract the device library (OCML) is written to.  Measured on the MI355X:
worst 0.594 ulp over all cases (0.500 on the specials and on quotients 1 +- 2^-k for k = 10 .. 52, 0.594 over thirty decades, 0.503
on the 2 100 000-cell tile); glibc's log on the same inputs: 0.500 ulp (tests/test_graph_fields.py).  The measured number is printed by every run and recorded in
DESIGN.md section 4.2; it is not asserted."""
import functools

import numpy as np
import pytest

import flowgraph_kit as K
import graph_fields as GF
from test_gpu_parity import ATOL, RTOL, assert_edge_set_equals_oracle

pytestmark = pytest.mark.gpu

LOG_ULPS = 3.0
CI_STATIC_MASK = 0x7FFF           # csrc/uca_graph.h: in-mask, out flags, pit flags, facet


def processor_of(F):
    """a fresh processor with the field's planes assigned"""
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=F.z.copy(), fill_flats=False, drain_pits_path=False, drain_pits=F.drain_pits, **F.spacing)
    dp.mag, dp.direction, dp.flats = F.mag.copy(), F.direction.copy(), F.flats.astype(bool)
    return dp


def run_uca(F):
    import warnings
    dp = processor_of(F)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp.calc_uca()
    return dp


def digest(dp):
    """what a second run of the same field must reproduce"""
    return (K.bits(np.asarray(dp.section, np.float64)), K.bits(dp.proportion), K.bits((dp._tile.graph_words() & CI_STATIC_MASK).astype(np.float64)),
            K.bits(np.asarray(dp.edge_todo, np.float64)), K.bits(np.asarray(dp.edge_done, np.float64)), K.bits(dp.uca))


def check_graph(F, dp, o, what):
    assert np.array_equal(dp.section, o.section), '%s: section differs in %d cells' % (what, (np.asarray(dp.section) != o.section).sum())
    K.assert_same_bits(dp.proportion, o.proportion, 'proportion, ' + what)
    words = dp._tile.graph_words()
    assert np.array_equal((words >> 12) & 7, o.section.astype(np.int64) & 7), what + ': facet field'
    return words


@pytest.mark.parametrize('field', GF.graph_fields(), ids=lambda f: f.name)
def test_calc_uca_on_assigned_directions(field):
    o = GF.oracle_of(field)
    dp = run_uca(field)
    what = field.name
    check_graph(field, dp, o, what)
    assert np.array_equal(dp.edge_todo, o.edge_todo), what + ': edge_todo'
    assert np.array_equal(dp.edge_done, o.edge_done), what + ': edge_done'
    assert_edge_set_equals_oracle(o, dp, exact=True)
    assert np.array_equal(np.asarray(dp.flats, bool), o.flats.astype(bool)), what + ': flats after the graph stage'
    uca, ref = np.asarray(dp.uca), o.uca
    assert np.array_equal(np.isnan(uca), np.isnan(ref)), what + ': NaN pattern of uca'
    assert np.isclose(uca, ref, rtol=RTOL, atol=ATOL, equal_nan=True).all(), what + ': uca'
    if field.drain_pits:
        pits = tuple(np.array(GF.PITS).T)
        assert not np.asarray(dp.flats)[pits].any() and (np.asarray(dp.section)[pits] == -1).all()     # patched mask, section of the mask before


@pytest.mark.parametrize('field', GF.graph_fields(), ids=lambda f: f.name)
def test_build_graph_on_assigned_directions(field):
    """the entry of a resumed directory job (pydem_build_graph): the same section and proportion bits and the same graph words"""
    import warnings
    o = GF.oracle_of(field)
    dp = processor_of(field)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp.build_graph()
    words = check_graph(field, dp, o, field.name + ', build_graph')
    assert_edge_set_equals_oracle(o, dp, exact=True)
    ref = run_uca(field)._tile.graph_words()
    assert np.array_equal(words & CI_STATIC_MASK, ref & CI_STATIC_MASK), field.name


def test_same_bits_in_a_child_under_poison():
    want = {f.name: digest(run_uca(f)) for f in GF.graph_fields()}
    body = "\n".join(["import test_gpu_graph_bits as T, graph_fields as GF",
                      "from pydem_amd import _ffi",
                      "for f in GF.graph_fields():",
                      "    print('BITS|%s|%s' % (f.name, '|'.join(T.digest(T.run_uca(f)))))",
                      "assert _ffi.poison_stats()[0] > 0",
                      "print('CHILD-OK')"])
    r = K.run_child(body, env={'PYDEM_MEM_POISON': '0xA5'}, timeout=300)
    for name, d in want.items():
        assert 'BITS|%s|%s' % (name, '|'.join(d)) in r.stdout, name


# ---- TWI -------------------------------------------------------------------------------------------------------------------
def device_twi(case):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=np.zeros(case.uca.shape), fill_flats=False, drain_pits_path=False, **case.options)
    dp.uca, dp.mag = case.uca.copy(), case.mag.copy()
    twi = dp.calc_twi()
    assert np.array_equal(dp.twi, twi * 10, equal_nan=True)
    return twi


@functools.lru_cache(maxsize=None)
def oracle_twi(case):
    from oracle import oracle as O
    return O.twi(case.uca, case.mag, case.min_slope, case.min_area, case.sat, case.lim_twi, case.lim_uca)


def check_twi(cases):
    worst = 0.0
    for c in cases:
        w, measured, capped = GF.twi_check(c, device_twi(c), oracle_twi(c), LOG_ULPS)
        print('%-34s worst %.4f ulp over %d cells, %d beyond the cap' % (c.name, w, measured, capped))
        assert w <= LOG_ULPS, '%s: the device logarithm is %.3f ulp off (bound %g)' % (c.name, w, LOG_ULPS)
        worst = max(worst, w)
    print('device log: worst %.4f ulp (bound %g)' % (worst, LOG_ULPS))
    return worst


def test_twi_on_the_small_cases():
    check_twi(GF.twi_cases(large=False))


def test_the_cap_is_applied_to_the_device_logarithm_exactly():
    """`t > twi_cap` on the device's own logarithm, without a tolerance: the capped plane is min(uncapped plane, cap) bit for bit, NaN
    kept.  The specials carry results 4 .. 1 ulp below the cap, at it and 1 .. 4 ulp above it (graph_fields.near_cap_quotient): a
    logarithm within LOG_ULPS is below the cap at -4 and above it at +4, so both sides of the comparison are met whatever the
    library returns in between; what it does return there is printed."""
    seen = 0
    for c in GF.twi_cases(large=False):
        if not c.lim_twi:
            continue
        cap = c.cap()
        free = device_twi(GF.TwiCase(c.name + ', no limit', c.uca, c.mag, c.min_slope, c.min_area, c.sat, False, c.lim_uca))
        got = device_twi(c)
        with np.errstate(invalid='ignore'):
            want = np.where(free > cap, cap, free)
        K.assert_same_bits(got, want, 'capped plane, ' + c.name)
        if c.name.startswith('specials') and np.isfinite(cap) and not c.lim_uca:
            near = np.abs(free - cap) <= 8 * np.spacing(cap)
            steps = np.sort(np.round((free[near] - cap) / np.spacing(cap)).astype(int))
            print('%s: uncapped results next to the cap, in ulp of it: %s' % (c.name, steps.tolist()))
            assert (free[near] < cap).any() and (free[near] > cap).any(), c.name
            assert (got[near] == cap).any() and (got[near] < cap).any() and not (got > cap).any(), c.name
            seen += 1
    assert seen >= 1


def test_twi_beyond_one_grid_of_threads():
    check_twi([GF.large_twi_case()])
