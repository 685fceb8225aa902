"""The designed graphs of cy_graphs.py on the CPU: the Python restatement of the two Cython loops and the oracle's C restatement
(oracle.drain_area / drain_connections) against the fixture that the reference's own Cython module wrote for them
(tests/golden/cy_graphs.npz, oracle/ref_harness/gen_golden_cyutils.py), to the bit; every case reaches its target and ends
under the model's round cap; and the start-of-round "snapshot" mutant of the model gives another answer where members of one
frontier push into each other in ascending order.  The two large cases are not in the fixture: model against oracle."""
import os

import numpy as np
import pytest

import cy_graphs as CG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cy_graphs.npz')
_cache = {}


def _case(name):
    """(case, the model's result, the fixture), each made once"""
    if 'fixture' not in _cache:
        d = np.load(GOLDEN)
        _cache['fixture'] = {k: d[k] for k in d.files}
    if name not in _cache:
        case = CG.CASES[name]()
        _cache[name] = (case, CG.run_model(case))
    return _cache[name] + (_cache['fixture'],)


def _fixture_out(fx, name, key):
    return fx.get('%s__out_%s' % (name, key))


@pytest.mark.parametrize('name', list(CG.CASES))
def test_case_ends_and_reaches_its_target(name):
    case, model, fx = _case(name)
    assert model is not None, "the model does not finish %s within %d rounds: not a case" % (name, CG.ROUND_CAP)
    assert CG.missed_facts(case, model) == []
    assert model['rounds'] == int(fx[name + '__rounds'])


@pytest.mark.parametrize('name', CG.SMALL)
def test_fixture_holds_the_inputs_of_the_case(name):
    case, _, fx = _case(name)
    for key in CG.INPUT_KEYS[case['kind']]:
        got = fx.get('%s__in_%s' % (name, key))
        if case[key] is None:
            assert got is None
        else:
            assert got is not None and np.array_equal(got, np.asarray(case[key])) and got.dtype == np.asarray(case[key]).dtype, key


@pytest.mark.parametrize('name', CG.SMALL)
def test_model_equals_fixture(name):
    case, model, fx = _case(name)
    assert model is not None
    keys = CG.AREA_KEYS if case['kind'] == 'area' else ('arr', 'ids')
    for key in keys:
        assert CG.same(model[key], _fixture_out(fx, name, key)), key


@pytest.mark.parametrize('name', CG.SMALL)
def test_oracle_equals_fixture(name):
    from oracle import oracle as O
    case, model, fx = _case(name)
    assert model is not None                         # only what the model finishes goes to compiled code
    got, _ = CG.call(O, case)
    for key, val in got.items():
        assert CG.same(val, _fixture_out(fx, name, key)), key


@pytest.mark.parametrize('name', CG.LARGE)
def test_model_equals_oracle_on_the_large_cases(name):
    from oracle import oracle as O
    case, model, _ = _case(name)
    assert model is not None
    got, _ = CG.call(O, case)
    for key, val in got.items():
        assert CG.same(val, model[key]), key


@pytest.mark.parametrize('name', ['loop2_plain', 'loop2_seeded', 'chain_up'])
def test_snapshot_mutant_differs(name):
    """the case tells "every push reads the current value" from "every push reads the value of the round's start\""""
    case, _, fx = _case(name)
    mutant = CG.run_model(case, snapshot=True)
    assert mutant is not None
    assert not np.array_equal(mutant['area'], _fixture_out(fx, name, 'area'))
    if case['edge_todo'] is not None:
        assert not np.array_equal(mutant['edge_todo'], _fixture_out(fx, name, 'edge_todo'))


def test_loop2_plain_numbers():
    """the worked example: 11 -> 12 (1), 12 -> 11 (0.5), 12 -> 13 (0.5), area = 1..25, both loop cells seeded"""
    case, model, fx = _case('loop2_plain')
    assert _fixture_out(fx, 'loop2_plain', 'area')[11:14].tolist() == [49.25, 49.5, 51.25]
    assert CG.run_model(case, snapshot=True)['area'][11:14].tolist() == [31.0, 43.5, 33.0]


def test_chain_down_is_one_step_per_round():
    """ids descending along the flow: no push reads a value written in its own round, so the mutant agrees there"""
    case, model, _ = _case('chain_down')
    assert CG.same(CG.run_model(case, snapshot=True)['area'], model['area'])


def test_fan_in_sum_order_shows():
    case, model, _ = _case('fan_in_300_taints')
    p = CG.fan_in_products(case)
    assert np.add.reduce(p) != np.add.reduce(p[::-1])
    t = 9 * 18 + 9
    fold = lambda q: np.cumsum(np.concatenate([[case['area'][t]], q]))[-1]          # one add after the other, as the loop does
    assert fold(p) != fold(p[::-1])
    first_round = fold(p)
    assert model['area'][t] == first_round


def test_csr_cases_are_what_they_say():
    from oracle import oracle as O
    c = CG.CASES['csr_duplicates']()
    rp, ri = O.tocsr(c['cp'], c['ci'], c['n_rows'] * c['n_cols'])
    assert np.array_equal(rp, c['rp']) and np.array_equal(ri, c['ri'])
    rows = [c['ri'][c['rp'][r]:c['rp'][r + 1]] for r in range(36)]
    assert sum(np.unique(r).size < r.size for r in rows) == 2
    u, f = CG.CASES['csr_unsorted'](), CG.CASES['loop_fed']()
    assert np.array_equal(u['rp'], f['rp']) and not np.array_equal(u['ri'], f['ri'])
    for r in range(49):
        a, b = u['rp'][r], u['rp'][r + 1]
        assert sorted(u['ri'][a:b]) == f['ri'][a:b].tolist()


@pytest.mark.parametrize('field', CG.SEQUENCE_FIELDS)
def test_call_sequence_driver_reproduces_the_oracle_chunk(field):
    """the driver around the capped model and around oracle.drain_area gives OracleDEM.calc_uca's uca and edge flags"""
    import warnings
    from oracle import oracle as O
    o, csr = CG.sequence_field(field)
    by_model = CG.uca_chunk_driver(o, csr, CG.model_as_drain_area)         # first: every call of the sequence ends
    by_oracle = CG.uca_chunk_driver(o, csr, O.drain_area)
    o = CG.sequence_field(field, built=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    for got in (by_model, by_oracle):
        assert np.array_equal(got[0], o.uca, equal_nan=True)
        assert np.array_equal(got[1], o.edge_todo) and np.array_equal(got[2], o.edge_done)
        assert got[3] == o.stats[0]
    if field != 'fractal_pits':
        assert o.stats[0] > 1, "the field is meant to need the re-seed"
