"""Cost of the horizon search (pydem_horizon) on the resident bench tile, next to the LDS-read floor of its design.

    python tools/horizon_cost.py [--size 16384] [--repeats 11] [--resources] [--out profiles/horizon_cost.txt]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning) and asks for the sky-view
factor alone, with edge_nan, at: 8 directions x 32 cells, 16 directions x 100 cells, and one direction x 100 cells (the cast
shadow).  Each: one cold call and `--repeats` warm ones into the same host array; the median, minimum and maximum of the warm
device times (a hipEvent pair around the kernels of the call; the table's upload and the download are not in it), the samples --
cells x steps of all rays, every lane takes every step whether its sample is on the tile or not -- and samples per second.  The
yardstick is the floor of the design, in which every sample is one 8-byte LDS read: samples x 8 B over the LDS read rate of the
chip, 256 CUs x 256 B per clock x 2.4 GHz = 157.3 TB/s; floor_ms and the ratio of the measured time to it stand beside each time.
--resources: registers, LDS and occupancy of the kernels from the compiler's report (a compile of csrc/horizon.hip alone; needs
no device; --size 0 skips the device part).  Appends one JSON line to `--out` and prints it."""
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

LDS_BYTES_PER_S = 256 * 256 * 2.4e9         # CUs x bytes per clock and CU (ds_read_b64) x clock
RUNS = (('svf_8_dirs_32_cells', 8, 32), ('svf_16_dirs_100_cells', 16, 100), ('shadow_1_dir_100_cells', 1, 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=11)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'horizon_cost.txt'))
    args = ap.parse_args()
    if args.size > 0 and args.repeats < 10:
        ap.error("--repeats must be at least 10: the figure is a median of warm runs")
    out = {}
    if args.resources:
        out['kernel_resources'] = kernel_resources('horizon.hip')
    if args.size > 0:
        from pydem_amd import DEMProcessor, horizon
        warnings.simplefilter('ignore')
        n = args.size
        cells = n * n
        dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
        tile = dp._ensure_tile()
        dp._push('elev')
        planes = {'svf': np.empty((n, n), np.float64)}
        runs = {}
        for label, n_dir, reach in RUNS:
            table = horizon.ray_table(n_dir, 0.0, reach * 30.0, 30.0, 30.0)
            steps = int(table.start[-1])
            ms = []
            for _ in range(args.repeats + 1):
                _, t, count = tile.horizon(table, True, False, True, out=planes)
                ms.append(t)
            warm = ms[1:]
            med, samples = statistics.median(warm), cells * steps
            floor = samples * 8 / LDS_BYTES_PER_S * 1e3
            runs[label] = dict(ms=round(med, 3), min=round(min(warm), 3), max=round(max(warm), 3), cold_ms=round(ms[0], 3), steps=steps,
                               samples=samples, Gsamples_per_s=round(samples / med / 1e6, 1), lds_floor_ms=round(floor, 3),
                               over_floor=round(med / floor, 2), n_defined=count)
            print('%s: %.3f ms' % (label, med), file=sys.stderr, flush=True)
        out.update(size=n, repeats=args.repeats, lds_TB_per_s=round(LDS_BYTES_PER_S / 1e12, 1), horizon=runs, device_bytes=tile.device_bytes())
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
