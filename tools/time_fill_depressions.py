"""Cost of the depression filling next to the plain sweep and the two other conditioning stages on the resident bench tile.

    python tools/time_fill_depressions.py [--size 16384] [--repeats 3] [--check-every N] [--no-conditioning]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m).  The fill is idempotent, so every call
gets a fresh synthetic surface (generated on the device).  For epsilon = 0 and the automatic epsilon: one call to load the
kernels and size the arena, then `--repeats` warm pydem_fill_depressions calls, depth not downloaded; device time of the call
(hipEvent pair) and its passes.  Then, in the same process and on the same surface: sweep_ms of one calc_uca, and calc_fill_flats
and run_pit_drain_paths, each timed on the host around a synchronised call as bench.py times them (they report no device time
of their own).  One JSON line per step, as it finishes.  --check-every sets PYDEM_FILL_CHECK_EVERY, the passes between two
looks at the change counter."""
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
    ap.add_argument('--check-every', type=int, default=None)
    ap.add_argument('--no-conditioning', action='store_true')
    args = ap.parse_args()
    if args.check_every is not None:
        os.environ['PYDEM_FILL_CHECK_EVERY'] = str(args.check_every)
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    tile = dp._tile

    def say(**kw):
        print(json.dumps(kw), flush=True)

    def fresh():
        tile.synth_fractal(seed=0)
        tile.synchronize()

    say(size=n, check_every=os.environ.get('PYDEM_FILL_CHECK_EVERY', 'default (4)'))
    for name, eps in (('eps_0', 0.0), ('eps_auto', None)):
        ms, wall, st = [], [], None
        for k in range(args.repeats + 1):
            fresh()
            t0 = time.perf_counter()
            _, used, n_raised, max_depth, passes, t = tile.fill_depressions(eps, None, False)
            dt = (time.perf_counter() - t0) * 1e3
            if k:                                   # (the first call loads the kernels and sizes the arena)
                ms.append(round(t, 3))
                wall.append(round(dt, 3))
            st = dict(epsilon=used, n_raised=n_raised, max_depth=max_depth, passes=passes)
        say(stage='fill_depressions', case=name, ms=ms, wall_ms=wall, **st)
    fresh()
    dp._on_device = {'elev'}
    dp.run_slopes_directions()
    dp.run_uca()
    tile.synchronize()
    tm = dp.timings
    say(stage='calc_uca', sweep_ms=round(tm['sweep_ms'], 3), slopes_directions_ms=round(tm['slopes_directions_ms'], 3),
        n_flats=tm['n_flats'], n_pits_undrained=tm['n_pits_undrained'])
    if args.no_conditioning:
        return
    for k in range(2):                              # (cold, then warm: the arena is sized by the first call)
        fresh()
        dp._on_device = {'elev'}
        t0 = time.perf_counter()
        dp.calc_fill_flats()
        tile.synchronize()
        t1 = time.perf_counter()
        dp.run_pit_drain_paths()
        tile.synchronize()
        t2 = time.perf_counter()
        say(stage='conditioning', run='warm' if k else 'cold', fill_flats_wall_ms=round((t1 - t0) * 1e3, 3),
            pit_drain_paths_wall_ms=round((t2 - t1) * 1e3, 3), elev_on_device='elev' in dp._on_device)


if __name__ == '__main__':
    main()
