"""Cost of the stream network (receivers, order and links, basins) next to the upslope distance and the upslope dependence on
the resident bench tile.

    python tools/time_stream_network.py [--size 16384] [--repeats 3] [--fraction 0.01] [--yardsticks]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once, takes
uca_threshold at the top `--fraction` of uca (the quantile of a seeded random sample of 2^22 cells), then runs pydem_stream_network
`--repeats` times warm with only the basins brought to the host (the forward sweep runs for them) and, with --yardsticks, in the
same process pydem_dist_up h/ave and the upslope dependence on the same streams.  Prints one line with the plain sweep's
sweep_ms, the device times of the receiver pass, the forward and the reverse sweep (hipEvent pairs), their levels
(PYDEM_DIST_DEBUG=1 prints what each schedule finished) and the switch point in force: PYDEM_DIST_MIN_PER_VISIT=<n> replaces
SN_FWD_MIN_PER_VISIT and SN_REV_MIN_PER_VISIT for the process, which is how the candidates are timed; `crc` is a checksum of the
basins, the same at every value.
"""
import argparse
import json
import os
import sys
import warnings
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--fraction', type=float, default=0.01)
    ap.add_argument('--yardsticks', action='store_true')
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    uca = np.asarray(dp.uca)
    sample = uca.ravel()[np.random.default_rng(0).integers(0, uca.size, 1 << 22)]
    thr = float(np.nanquantile(sample, 1.0 - args.fraction))
    with np.errstate(invalid='ignore'):
        streams = uca >= thr
    dp._host.pop('uca', None)
    del uca
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'min_per_visit': os.environ.get('PYDEM_DIST_MIN_PER_VISIT', 'default'),
           'uca_threshold': thr, 'stream_fraction': round(float(streams.mean()), 5)}
    call = lambda: dp._tile.stream_network(None, thr, receiver=False, order=False, link=False, basin=True)
    call()                                        # first call: allocates the planes, loads the kernels
    ms = []
    for _ in range(args.repeats):
        planes, t, levels, left = call()
        ms.append(t)
    out.update(receiver_ms=[round(t[0], 3) for t in ms], forward_ms=[round(t[1], 3) for t in ms], reverse_ms=[round(t[2], 3) for t in ms],
               levels=levels, n_unresolved=left, crc=zlib.crc32(planes['basin']))
    if args.yardsticks:
        for name, f in (('up_h_ave', lambda: dp._tile.dist_up('h', 'ave', True, download=False)),
                        ('dependence', lambda: dp._tile.rev_accum('sum', None, streams, 1.0, download=False))):
            f()
            res = [f() for _ in range(args.repeats)]
            out[name] = dict(ms=[round(r[1], 3) for r in res], levels=res[-1][2])
    assert dp.timings['sweep_ms'] == sweep_ms
    print(json.dumps(out))


if __name__ == '__main__':
    main()
