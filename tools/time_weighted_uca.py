"""Cost of the weighted flow accumulation next to the plain sweep on the resident bench tile.

    python tools/time_weighted_uca.py [--size 16384] [--repeats 3]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once,
then run_weighted_uca `--repeats` times warm (random weights in [-1, 2], fixed seed) and prints one line with the plain
sweep's sweep_ms and every uca_weighted_ms (pydem_timings: seed + level re-arm + weighted schedule, hipEvent pairs).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.calc_uca()
    sweep_ms = dp.timings['sweep_ms']
    w = np.random.default_rng(0).uniform(-1.0, 2.0, (n, n))
    dp.run_weighted_uca(w)                     # first call: allocates the weight / result planes
    ms = []
    for _ in range(args.repeats):
        dp.run_weighted_uca(w)
        ms.append(dp.timings['uca_weighted_ms'])
        assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps({'size': n, 'sweep_ms': round(sweep_ms, 3), 'uca_weighted_ms': [round(v, 3) for v in ms],
                      'ratio_median': round(float(np.median(ms)) / sweep_ms, 3)}))


if __name__ == '__main__':
    main()
