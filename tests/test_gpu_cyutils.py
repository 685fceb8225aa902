"""The cyutils-compatible boundary (pydem_amd.cyfuncs.cyutils, csrc/cyutils.hip) against the oracle's
restatement of cyutils._drain_area / _drain_connections (itself pinned bit-exact through the UCA goldens),
on real flow graphs built from seeded tiles: same call sequence as the reference's _calc_uca_chunk
(dem_processing.py:879-960) and _calc_uca_chunk_update (:820-853)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _graph(shape, seed, pits):
    from oracle import oracle as O
    from pydem_amd import synth
    elev = synth.fractal(shape[0], shape[1], seed=seed, top_shift=6, n_octaves=6)
    o = O.OracleDEM(elev, dX=30.0, dY=30.0, drain_pits=pits)
    o.calc_slopes_directions(); o.build_graph()
    indptr, indices, data = o.A
    rp, ri = O.tocsr(indptr, indices, elev.size)
    return o, (indptr, indices, data, rp, ri)


@pytest.mark.parametrize('shape,seed,pits', [((120, 90), 51, False), ((200, 260), 52, True)])
def test_drain_area_matches_oracle(shape, seed, pits):
    from oracle import oracle as O
    from pydem_amd.cyfuncs import cyutils
    o, (cp, ci, cd, rp, ri) = _graph(shape, seed, pits)
    n, m = shape
    N = n * m
    insum = np.zeros(N); np.add.at(insum, ci, cd)
    ids0 = insum == 0
    rng = np.random.default_rng(seed)
    et0 = (rng.random(N) < 0.01).astype(float)

    def fresh():
        return (np.repeat(900.0, N), ids0.copy(), ids0.copy(), et0.copy(), et0.copy())
    a1, d1, i1, e1, f1 = fresh()
    O.drain_area(a1, d1, i1, cp, ci, cd, rp, ri, n, m, e1, f1)
    a2, d2, i2, e2, f2 = fresh()
    cyutils.drain_area(a2, d2, i2, cp, ci, cd, rp, ri, n, m, e2, f2)
    assert np.array_equal(d1, d2)
    # additions into a target follow the Cython order (ascending source id, no floating-point atomics): bit for bit
    assert np.array_equal(a2, a1)
    assert np.array_equal(e2, e1) and np.array_equal(f2, f1)
    a3, d3, i3, e3, f3 = fresh()
    cyutils.drain_area(a3, d3, i3, cp, ci, cd, rp, ri, n, m, e3, f3)
    assert np.array_equal(a3, a2) and np.array_equal(e3, e2)          # and run to run
    # skip_edge variant without the taint arrays (the edge-update call, :836-842)
    a1, d1, i1, _, _ = fresh(); a2, d2, i2, _, _ = fresh()
    O.drain_area(a1, d1, i1, cp, ci, cd, rp, ri, n, m, skip_edge=1)
    cyutils.drain_area(a2, d2, i2, cp, ci, cd, rp, ri, n, m, skip_edge=1)
    assert np.array_equal(d1, d2)
    assert np.array_equal(a2, a1)


@pytest.mark.parametrize('shape,seed,pits', [((150, 110), 53, True)])
def test_drain_connections_matches_oracle(shape, seed, pits):
    from oracle import oracle as O
    from pydem_amd.cyfuncs import cyutils
    o, (cp, ci, cd, rp, ri) = _graph(shape, seed, pits)
    N = shape[0] * shape[1]
    rng = np.random.default_rng(seed)
    for set_to in (False, True):
        arr = np.full(N, not set_to)
        ids = rng.random(N) < 0.002
        a1, a2 = arr.copy(), arr.copy()
        O.drain_connections(a1, ids.copy(), cp, ci, set_to=set_to)
        cyutils.drain_connections(a2, ids.copy(), cp, ci, set_to=set_to)
        assert np.array_equal(a1, a2)
        assert (a1 == set_to).sum() > 0


# --- designed graphs (tests/cy_graphs.py): frontiers whose members push into each other, edge rules, CSR forms, wide frontiers ---

def _designed_failures(names=None):
    """Every designed case through the shim, twice: against the reference's fixture (the large cases: against the oracle alone)
    and against the oracle, array_equal on everything the call updates or returns.  -> list of 'case: what differs'"""
    import os
    import cy_graphs as CG
    from oracle import oracle as O
    from pydem_amd.cyfuncs import cyutils
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cy_graphs.npz'))
    fx = {k: d[k] for k in d.files}
    bad = []
    for name in names or list(CG.CASES):
        case = CG.CASES[name]()
        # only a case that the capped model has finished (its round count is on record) goes to the oracle and the device
        assert 0 < int(fx[name + '__rounds']) <= CG.ROUND_CAP
        want, _ = CG.call(O, case)
        runs = [CG.call(cyutils, case) for _ in range(2)]
        for r, (got, ret) in enumerate(runs):
            for key, val in got.items():
                if not CG.same(val, want[key]):
                    bad.append('%s: run %d, %s differs from the oracle' % (name, r, key))
                if name not in CG.LARGE and not CG.same(val, fx.get('%s__out_%s' % (name, key))):
                    line = '%s: run %d, %s differs from the fixture' % (name, r, key)
                    if name.startswith('loop2') and key == 'area':
                        line += ' (cells 11, 12, 13: got %r, wanted %r)' % (val[11:14].tolist(), fx[name + '__out_area'][11:14].tolist())
                    bad.append(line)
            if name in CG.LARGE:
                continue
            # what the call returns: the arrays it was given (a stand-in of one zero for a taint array that was left out)
            ret = ret if isinstance(ret, tuple) else (ret,)
            n_ret = sum(1 for k in fx if k.startswith(name + '__ret_'))
            if len(ret) != n_ret:
                bad.append('%s: run %d returns %d objects, the reference %d' % (name, r, len(ret), n_ret))
                continue
            for k, val in enumerate(ret):
                w = fx['%s__ret_%d' % (name, k)]
                if val is None or np.asarray(val).dtype != w.dtype or not np.array_equal(np.asarray(val), w):
                    bad.append('%s: run %d, returned object %d differs from the fixture' % (name, r, k))
            if case['kind'] == 'area' and not (ret[0] is got['area'] and ret[1] is got['done']):
                bad.append('%s: run %d does not return the arrays it was given' % (name, r))
            if case['kind'] == 'conn' and ret[0] is not got['arr']:
                bad.append('%s: run %d does not return the array it was given' % (name, r))
        for key in runs[0][0]:
            if not CG.same(runs[0][0][key], runs[1][0][key]):
                bad.append('%s: %s differs run to run' % (name, key))
    return bad


def test_designed_graphs_match_fixture_and_oracle():
    """One child process under a time limit: a shim that does not stop must not hold the suite.  The recorded round counts are
    at most 7 and a round is a few launches, so the small cases take milliseconds each; the two 2050 x 512 cases move ~100 MB
    each way and dominate.  30 s is two orders of magnitude above the rounds and still seconds."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "import test_gpu_cyutils as T\n"
              "bad = T._designed_failures()\n"
              "print('\\n'.join(bad)); print('CY-DONE', len(bad))\n") % (root, os.path.join(root, 'tests'))
    r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=30, cwd=root)
    assert r.returncode == 0 and 'CY-DONE 0' in r.stdout, r.stdout[:4000] + ' ... ' + r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize('field', ['two_cells', 'three_cells', 'two_loops', 'fractal_pits'])
def test_call_sequence_through_the_shim(field):
    """The reference's stall / re-seed loop (cy_graphs.uca_chunk_driver, pinned to OracleDEM.calc_uca on the CPU) with the shim
    as its drain_area against the same loop with the oracle's, to the bit.  On the level fields the re-seed puts both cells of
    a loop into one frontier.  The capped model goes first: the sequence reaches the device only if every call of it ends."""
    import cy_graphs as CG
    from oracle import oracle as O
    from pydem_amd.cyfuncs import cyutils
    o, csr = CG.sequence_field(field)
    CG.uca_chunk_driver(o, csr, CG.model_as_drain_area)
    want = CG.uca_chunk_driver(o, csr, O.drain_area)
    got = CG.uca_chunk_driver(o, csr, cyutils.drain_area)
    if field != 'fractal_pits':
        assert want[3] > 1, "the field is meant to need the re-seed"
    assert got[3] == want[3]
    assert np.array_equal(got[0], want[0], equal_nan=True)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
