"""Cost of the HAND hydraulic table (pydem_hand_table) on the resident bench tile, next to the sweeps it follows.

    python tools/hand_hydraulics_cost.py [--size 16384] [--repeats 3] [--fraction 0.001] [--stages 32] [--numpy] [--resources]
                                         [--out profiles/hand_hydraulics_cost.txt]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once and takes
uca_threshold at the top `--fraction` of uca (the quantile of a seeded random sample of 2^22 cells).  For scale: one calc_hand and
one calc_stream_network(basins=True) on those streams, wall time and the device time of their sweeps.  Then, with the basin plane
as the zones and `--stages` stages at evenly spaced quantiles of the finite HAND, pydem_hand_table once cold and `--repeats` times
warm each way: with the HAND plane as pydem_dist_down left it on the device, and with the host copy of it (the upload of 8 B per
cell is then part of the wall time; the zone plane, 4 B per cell, is uploaded either way).  Per call the device time of the two
kernels (hipEvent pairs) and the wall time; both ways must return the same bytes.  --numpy: the same table on the host (one
searchsorted, four bincounts with float weights), wall time, once.  --resources: registers, LDS and occupancy of the two kernels
from the compiler's report (a compile of csrc/hand_table.hip alone; needs no device).  Appends one JSON line to `--out` and prints
it."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources      # (tools/ is the script directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--fraction', type=float, default=0.001)
    ap.add_argument('--stages', type=int, default=32)
    ap.add_argument('--numpy', action='store_true')
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hand_hydraulics_cost.txt'))
    args = ap.parse_args()
    out = {}
    if args.resources:
        out['kernel_resources'] = kernel_resources('hand_table.hip')
    if args.size > 0:
        from pydem_amd import DEMProcessor
        warnings.simplefilter('ignore')
        n = args.size
        dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
        dp.run_slopes_directions()
        dp.run_uca()
        uca = np.asarray(dp.uca)
        sample = uca.ravel()[np.random.default_rng(0).integers(0, uca.size, 1 << 22)]
        thr = float(np.nanquantile(sample, 1.0 - args.fraction))
        dp._host.pop('uca', None)
        del uca
        out.update(size=n, sweep_ms=round(dp.timings['sweep_ms'], 3), uca_threshold=thr)
        t0 = time.perf_counter()
        hand = dp.calc_hand(uca_threshold=thr)
        out['calc_hand'] = dict(wall_s=round(time.perf_counter() - t0, 2), ms=round(dp.dist_down_stats['ms'], 3))
        t0 = time.perf_counter()
        net = dp.calc_stream_network(uca_threshold=thr, basins=True)
        out['calc_stream_network'] = dict(wall_s=round(time.perf_counter() - t0, 2), ms=[round(t, 3) for t in dp.stream_network_stats['ms']])
        zone, K = net.basin, int(net.links.size)
        sample = hand.ravel()[np.random.default_rng(1).integers(0, hand.size, 1 << 22)]
        stages = np.unique(np.quantile(sample[np.isfinite(sample)], np.linspace(0.02, 0.9, args.stages)))
        out.update(n_links=K, n_stages=int(stages.size), table_bytes=(K * int(stages.size) * 4 + K * 2) * 8,
                   in_a_basin=round(float((zone >= 1).mean()), 4))
        tile = dp._tile
        tile.dist_down('v', 'ave', None, thr, download=False)           # the resident plane (calc_stream_network took it)
        results = {}
        for name, plane in (('resident', None), ('host_plane', hand)):
            calls = []
            for k in range(args.repeats + 1):
                t0 = time.perf_counter()
                ints, skipped, quanta, ms = tile.hand_table(zone, stages, K, hand=plane)
                calls.append(dict(wall_ms=round((time.perf_counter() - t0) * 1e3, 2), **{p: round(v, 3) for p, v in ms.items()}))
            results[name] = (ints, skipped, quanta)
            out[name] = dict(cold=calls[0], warm=calls[1:])
        a, b = results['resident'], results['host_plane']
        out['same_bytes'] = bool(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2])
        out.update(cells_counted=int(a[0][:, :, 0].sum()), cells_nan=int(a[1][:, 0].sum()), cells_above=int(a[1][:, 1].sum()), quanta=a[2])
        if args.numpy:
            t0 = time.perf_counter()
            zf, hf = zone.ravel(), hand.ravel()
            with np.errstate(invalid='ignore'):
                c = np.flatnonzero((zf >= 1) & (hf <= stages[-1]))
            key = (zf[c].astype(np.int64) - 1) * stages.size + np.searchsorted(stages, hf[c], 'left')
            area = np.full(c.size, 900.0)
            slope = np.sqrt(1.0 + np.asarray(dp.mag).ravel()[c] ** 2)
            cols = [np.bincount(key, minlength=K * stages.size)] + [np.bincount(key, weights=w, minlength=K * stages.size)
                                                                    for w in (area, area * hf[c], area * slope)]
            out['numpy'] = dict(wall_s=round(time.perf_counter() - t0, 2), cells_equal=bool(np.array_equal(cols[0].reshape(K, -1), a[0][:, :, 0])))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
