"""Cost of the depression inventory next to the fill it shares its relaxation with, on the resident bench tile.

    python tools/time_depressions.py [--size 16384] [--repeats 3] [--no-labels]

Builds the tile like bench.py and tools/time_fill_depressions.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m).  One
pydem_depressions call to load the kernels and size the arena, then `--repeats` warm calls: device time of the call and of its
parts (hipEvent pairs: relaxation, marking + block-local labelling, seam merge, flatten, numbering, statistics, label write), K,
the largest depression.  The inventory does not change the surface, so every call sees the same one.  Then the same under
PYDEM_DEPR_LOCAL=0 when --size is at most 4096 (every union through the global merge), and, as the yardstick, the default-schedule
eps = 0 timings of pydem_fill_depressions in the same process, each on a fresh synthetic surface.  One JSON line per step."""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-labels', action='store_true')
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    tile = dp._tile

    def say(**kw):
        print(json.dumps(kw), flush=True)

    def inventory(case):
        parts, wall, st = {}, [], None
        for k in range(args.repeats + 1):
            t0 = time.perf_counter()
            label, rows, info = tile.depressions(want_labels=not args.no_labels)
            dt = (time.perf_counter() - t0) * 1e3
            if k:                                   # (the first call loads the kernels and sizes the arena)
                for nm, v in info['ms'].items():
                    parts.setdefault(nm, []).append(round(v, 3))
                wall.append(round(dt, 3))
            st = dict(K=info['n_found'], largest_cells=int(rows['cells'].max()) if len(rows) else 0,
                      raised_cells=int(rows['cells'].sum()), single_cell=int((rows['cells'] == 1).sum()),
                      max_depth=float(rows['max_depth'].max()) if len(rows) else 0.0, passes=info['passes'], quanta=info['quanta'])
            del label, rows
        say(stage='depressions', case=case, ms=parts, wall_ms=wall, **st)

    say(size=n, labels=not args.no_labels)
    tile.synth_fractal(seed=0)
    tile.synchronize()
    inventory('default')
    if n <= 4096:
        os.environ['PYDEM_DEPR_LOCAL'] = '0'
        inventory('PYDEM_DEPR_LOCAL=0')
        del os.environ['PYDEM_DEPR_LOCAL']
    ms, st = [], None
    for k in range(args.repeats + 1):
        tile.synth_fractal(seed=0)
        tile.synchronize()
        _, used, n_raised, max_depth, passes, t = tile.fill_depressions(0.0, None, False)
        if k:
            ms.append(round(t, 3))
        st = dict(epsilon=used, n_raised=n_raised, max_depth=max_depth, passes=passes)
    say(stage='fill_depressions', case='eps_0', ms=ms, **st)


if __name__ == '__main__':
    main()
