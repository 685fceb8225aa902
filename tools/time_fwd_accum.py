"""Cost of the forward accumulation (decaying, transport-limited) next to the upslope distance and the reverse accumulation on the
resident bench tile.

    python tools/time_fwd_accum.py [--size 16384] [--repeats 3] [--checksum]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once, then
runs pydem_fwd_accum `--repeats` times warm for a random load without mult (decay), with mult in [0.5, 1] (decay_mult) and for
a supply under a capacity with the inflow pass (trans_lim: supply U(0, 2), capacity 5 x U(0.5, 1.5)), and in
the same process pydem_dist_up h/ave and pydem_rev_accum op 0 on the same load (the yardsticks: the same graph, the same
engine).  Prints one line with the plain sweep's sweep_ms, every call's device time (hipEvent pairs; trans_lim: sweep + inflow
pass), its levels (the initial one + tile passes + queue levels; PYDEM_DIST_DEBUG=1 prints what each schedule finished) and the
ratio of the medians to dist_up's.  The device time of a call does not include the upload of its planes.  PYDEM_DIST_MIN_PER_VISIT
=<n> moves the switch point of every sweep in the process; --checksum adds the sha256 of the decay_mult result and of the
transport and the inflow, which must not depend on it.
"""
import argparse
import hashlib
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, repeats, pick):
    call()                                        # first call: allocates the planes, loads the kernels
    ms, lv, left = [], 0, 0
    for _ in range(repeats):
        t, lv, left = pick(call())
        ms.append(t)
    return dict(ms=[round(v, 3) for v in ms], levels=lv, n_unresolved=left)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--checksum', action='store_true')
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    dp._host.pop('uca', None)
    rng = np.random.default_rng(0)
    load = rng.uniform(-1.0, 2.0, (n, n))
    mult = rng.uniform(0.5, 1.0, (n, n))
    supply = rng.uniform(0.0, 2.0, (n, n))
    cap = 5.0 * rng.uniform(0.5, 1.5, (n, n))
    t = dp._tile
    fwd, other = (lambda r: (r[2], r[3], r[4])), (lambda r: (r[1], r[2], r[3]))
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'min_per_visit': os.environ.get('PYDEM_DIST_MIN_PER_VISIT', 'default')}
    out['decay'] = timed(lambda: t.fwd_accum(load, None, None, True, download=False), args.repeats, fwd)
    out['decay_mult'] = timed(lambda: t.fwd_accum(load, mult, None, True, download=False), args.repeats, fwd)
    out['trans_lim'] = timed(lambda: t.fwd_accum(supply, None, cap, True, inflow=True, download=False), args.repeats, fwd)
    out['trans_lim_no_inflow'] = timed(lambda: t.fwd_accum(supply, None, cap, True, download=False), args.repeats, fwd)
    out['up_h_ave'] = timed(lambda: t.dist_up('h', 'ave', True, download=False), args.repeats, other)
    out['racc'] = timed(lambda: t.rev_accum('sum', load, None, download=False), args.repeats, other)
    up = float(np.median(out['up_h_ave']['ms']))
    for name in ('decay', 'decay_mult', 'trans_lim', 'trans_lim_no_inflow', 'racc'):
        out[name]['ratio_to_up'] = round(float(np.median(out[name]['ms'])) / up, 3)
    if args.checksum:
        out['sha_decay_mult'] = sha(t.fwd_accum(load, mult, None, True)[0])
        v, flow = t.fwd_accum(supply, None, cap, True, inflow=True)[:2]
        out['sha_trans_lim'] = [sha(v), sha(flow)]
        out['deposit_fraction'] = round(float(np.mean((supply + flow) - v > 0)), 4)
    assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps(out))


if __name__ == '__main__':
    main()
