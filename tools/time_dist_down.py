"""Cost of the downslope distance / HAND next to the plain sweep on the resident bench tile.

    python tools/time_dist_down.py [--size 16384] [--repeats 3] [--cells 500] [--ramp 8192]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once,
then pydem_dist_down `--repeats` times warm for h/ave and v/ave (HAND) with the streams at `--cells` cells, without bringing
the result to the host, and prints one line with the plain sweep's sweep_ms and every call's device time (hipEvent pair),
and its levels (the initial one + tile passes + queue levels; PYDEM_DIST_DEBUG=1 prints what each schedule finished).  --ramp N (0 = off): the same for a target at the foot of an N x N ramp
(z = 2000 - 1.5 row + 10 sin(col / 37) row / N + noise, target = the last two rows), where the reverse depth is the tile's
length.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

def timed(dp, repeats, kind, **target):
    dp._tile.dist_down(kind, 'ave', download=False, **target)            # first call: allocates the call's planes
    ms, lv, left = [], 0, 0
    for _ in range(repeats):
        _, t, lv, left = dp._tile.dist_down(kind, 'ave', download=False, **target)
        ms.append(t)
    return dict(ms=[round(v, 3) for v in ms], levels=lv, n_unresolved=left)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cells', type=float, default=500.0)
    ap.add_argument('--ramp', type=int, default=8192)
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'cells': args.cells}
    for name, kind in (('h_ave', 'h'), ('hand', 'v')):
        r = timed(dp, args.repeats, kind, uca_threshold=args.cells * 900.0)
        r['ratio_median'] = round(float(np.median(r['ms'])) / sweep_ms, 3)
        out[name] = r
    assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps(out))
    del dp
    if args.ramp:
        n = args.ramp
        row, col = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
        z = 2000 - 1.5 * row + 10 * np.sin(col / 37) * row / n + np.random.default_rng(1).normal(0, 0.4, (n, n))
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
        dp.run_slopes_directions()
        dp.run_uca()
        target = np.zeros((n, n), bool)
        target[-2:] = True
        r = timed(dp, args.repeats, 'h', target=target)
        print(json.dumps({'ramp': n, 'sweep_ms': round(dp.timings['sweep_ms'], 3), 'h_ave': r}))


if __name__ == '__main__':
    main()
