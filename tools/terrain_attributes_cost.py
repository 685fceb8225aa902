"""Cost of the terrain attributes (pydem_terrain_attributes) on the resident bench tile, next to a streaming kernel of the same box.

    python tools/terrain_attributes_cost.py [--size 16384] [--repeats 11] [--resources] [--out profiles/terrain_attributes_cost.txt]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning) and runs the pipeline up to
calc_twi once, so that pydem_twi can be timed on the same tile in the same process: `--repeats` warm calls, the median of its
device time (twi_ms) and the bytes it must move (uca and mag read, twi written: 24 B per cell) -- the yardstick.  Then, for the
windows 3 and 15, each with 'gradient' alone and with all nine planes: one cold call and `--repeats` warm ones into the same host
arrays, the median, minimum and maximum of the warm device times (a hipEvent pair around the kernel; the downloads are not in
it), the bytes the call must move (8 B read + 8 B per plane written, per cell), the rate that makes, and the time per byte over
the yardstick's.  --resources: registers, LDS and occupancy of the kernels from the compiler's report (a compile of
csrc/terrain.hip alone; needs no device; --size 0 skips the device part).  Appends one JSON line to `--out` and prints it."""
import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources      # (tools/ is the script directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=11)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'terrain_attributes_cost.txt'))
    args = ap.parse_args()
    if args.size > 0 and args.repeats < 10:
        ap.error("--repeats must be at least 10: the figure is a median of warm runs")
    out = {}
    if args.resources:
        out['kernel_resources'] = kernel_resources('terrain.hip')
    if args.size > 0:
        from pydem_amd import DEMProcessor, terrain
        warnings.simplefilter('ignore')
        n = args.size
        cells = n * n
        dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
        dp.run_twi()
        twi = []
        for _ in range(args.repeats):
            dp.run_twi()
            twi.append(dp.timings['twi_ms'])
        y_ms, y_bytes = statistics.median(twi), 24 * cells
        out.update(size=n, repeats=args.repeats,
                   pydem_twi=dict(ms=round(y_ms, 3), min=round(min(twi), 3), max=round(max(twi), 3), bytes=y_bytes,
                                  GB_per_s=round(y_bytes / y_ms / 1e6, 1)))
        tile = dp._tile
        light = terrain.light_vector(315.0, 45.0)
        planes = {nm: np.empty((n, n), np.float64) for nm in terrain.ATTRIBUTES}
        runs = {}
        for window in (3, 15):
            for label, which in (('gradient', ('gradient',)), ('all_nine', terrain.ATTRIBUTES)):
                ms = []
                for _ in range(args.repeats + 1):
                    _, t, count = tile.terrain_attributes(which, window // 2, light, 1.0, out=planes)
                    ms.append(t)
                warm = ms[1:]
                med, moved = statistics.median(warm), (8 + 8 * len(which)) * cells
                runs['window_%d_%s' % (window, label)] = dict(
                    ms=round(med, 3), min=round(min(warm), 3), max=round(max(warm), 3), cold_ms=round(ms[0], 3), bytes=moved,
                    GB_per_s=round(moved / med / 1e6, 1), per_byte_over_twi=round((med / moved) / (y_ms / y_bytes), 2), n_defined=count)
                print('window %d %s: %.3f ms' % (window, label, med), file=sys.stderr, flush=True)
        out['terrain_attributes'] = runs
        out['device_bytes'] = tile.device_bytes()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
