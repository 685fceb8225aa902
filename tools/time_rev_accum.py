"""Cost of the reverse accumulation (upslope dependence, racc, dmax) next to the downslope distance on the resident bench tile.

    python tools/time_rev_accum.py [--size 16384] [--repeats 3] [--cells 500]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once, takes
the streams at `--cells` cells as the target set, then runs pydem_rev_accum `--repeats` times warm for the dependence on the
streams (op 0, absorb = streams), racc and dmax of a random load (op 0 / op 1, seed = load) without bringing the result to the
host, and in the same process pydem_dist_down h/ave on the same target mask (the yardstick: it finishes the same open set over
the same edges with the same schedule).  Prints one line with the plain sweep's sweep_ms, every call's device time (hipEvent
pair), its levels (the initial one + tile passes + queue levels; PYDEM_DIST_DEBUG=1 prints what each schedule finished) and the
ratio of the medians.  The device time of a call with a seed or a mask does not include their upload.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, repeats):
    call()                                        # first call: allocates the planes, loads the kernels
    ms, lv, left = [], 0, 0
    for _ in range(repeats):
        _, t, lv, left = call()
        ms.append(t)
    return dict(ms=[round(v, 3) for v in ms], levels=lv, n_unresolved=left)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cells', type=float, default=500.0)
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    target = np.asarray(dp.uca) >= args.cells * 900.0
    dp._host.pop('uca', None)
    load = np.random.default_rng(0).uniform(-1.0, 2.0, (n, n))
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'cells': args.cells, 'target_fraction': round(float(target.mean()), 5)}
    out['dependence'] = timed(lambda: dp._tile.rev_accum('sum', None, target, 1.0, download=False), args.repeats)
    out['racc'] = timed(lambda: dp._tile.rev_accum('sum', load, None, download=False), args.repeats)
    out['dmax'] = timed(lambda: dp._tile.rev_accum('max', load, None, download=False), args.repeats)
    out['down_h_ave'] = timed(lambda: dp._tile.dist_down('h', 'ave', target=target, download=False), args.repeats)
    down = float(np.median(out['down_h_ave']['ms']))
    for name in ('dependence', 'racc', 'dmax'):
        out[name]['ratio_to_down'] = round(float(np.median(out[name]['ms'])) / down, 3)
    assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps(out))


if __name__ == '__main__':
    main()
