"""Cost of the upslope flow-path distance next to the plain sweep and the downslope distance on the resident bench tile.

    python tools/time_dist_up.py [--size 16384] [--repeats 3] [--cells 500] [--no-edge-nan]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once, then
pydem_dist_up `--repeats` times warm for h/max and h/ave without bringing the result to the host, and in the same process
pydem_dist_down h/ave with the streams at `--cells` cells (the yardstick: it finishes the same cells over the same edges).
Prints one line with the plain sweep's sweep_ms, every call's device time (hipEvent pair), its levels (the initial one + tile
passes + queue levels; PYDEM_DIST_DEBUG=1 prints what each schedule finished) and the ratio of the medians.
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
    ap.add_argument('--no-edge-nan', action='store_true')
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    edge_nan = not args.no_edge_nan
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'cells': args.cells, 'edge_nan': edge_nan}
    for name, stat in (('up_h_max', 'max'), ('up_h_ave', 'ave')):
        out[name] = timed(lambda: dp._tile.dist_up('h', stat, edge_nan, download=False), args.repeats)
    out['down_h_ave'] = timed(lambda: dp._tile.dist_down('h', 'ave', uca_threshold=args.cells * 900.0, download=False), args.repeats)
    down = float(np.median(out['down_h_ave']['ms']))
    for name in ('up_h_max', 'up_h_ave'):
        out[name]['ratio_to_down'] = round(float(np.median(out[name]['ms'])) / down, 3)
        out[name]['ratio_to_sweep'] = round(float(np.median(out[name]['ms'])) / sweep_ms, 3)
    assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps(out))


if __name__ == '__main__':
    main()
