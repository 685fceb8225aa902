#!/usr/bin/env python
"""Golden vectors for the cyutils boundary: the designed graphs of tests/cy_graphs.py (all but the two large ones) through the
UNMODIFIED Cython module of the reference, drain_area and drain_connections.  Written to tests/golden/cy_graphs.npz: every
case's inputs, the arrays after the call (area, done, ids, the taints / arr), what the call returned, and the round count of
the Python model, which also runs the large cases.  A case goes to the compiled module only after the model, which stops at a
round cap, has finished it: the Cython loops do not end on every input.  Run through run.sh."""
import hashlib
import os
import sys

from load_reference import load_reference

pydem = load_reference()
import numpy as np  # noqa: E402
from pydem.cyfuncs import cyutils  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import cy_graphs as CG  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')


def main():
    rec = {}
    for name, make in CG.CASES.items():
        case = make()
        model = CG.run_model(case)
        missed = CG.missed_facts(case, model)
        assert not missed, (name, missed)
        rec[name + '__rounds'] = np.int64(model['rounds'])
        if name in CG.LARGE:
            continue
        for key in CG.INPUT_KEYS[case['kind']]:
            if case[key] is not None:
                rec['%s__in_%s' % (name, key)] = np.asarray(case[key])
        got, ret = CG.call(cyutils, case)
        for key, val in got.items():
            if val is not None:
                rec['%s__out_%s' % (name, key)] = val
        for k, val in enumerate(ret if isinstance(ret, tuple) else (ret,)):
            rec['%s__ret_%d' % (name, k)] = np.asarray(val)
        same = all(CG.same(got[k], model[k]) for k in got)
        print('%-24s rounds %d  model == reference: %s' % (name, model['rounds'], same))
    np.savez_compressed(os.path.join(OUT, 'cy_graphs.npz'), **rec)
    # this fixture's line of the manifest
    lines = [ln for ln in open(os.path.join(OUT, 'SHA256SUMS')).read().splitlines() if ln and ln.split()[1] != 'cy_graphs.npz']
    lines.append('%s  cy_graphs.npz' % hashlib.sha256(open(os.path.join(OUT, 'cy_graphs.npz'), 'rb').read()).hexdigest())
    open(os.path.join(OUT, 'SHA256SUMS'), 'w').write('\n'.join(sorted(lines, key=lambda ln: ln.split()[1])) + '\n')


if __name__ == '__main__':
    main()
