"""Cost of the fill across tiles (ProcessManager.process_fill_depressions) next to the per-tile fill on the same tiles.

    python tools/fill_mosaic_cost.py [--size 8192] [--out profiles/fill_mosaic_cost.txt]
    python tools/fill_mosaic_cost.py --compiler-report [--out profiles/fill_mosaic_cost.txt]      (no GPU needed)

The mosaic is bench.py's layout: 2 x 4 tiles of --size^2 with a one-pixel overlap, elevations from the device generator at global
mosaic coordinates, all on GPU 0.  For epsilon = 0 and the automatic epsilon: one run on a mosaic of its own to load the kernels and
size the arena, then on a fresh mosaic the rounds of process_fill_depressions (tiles relaxed, cells that fell, passes, device ms
summed over the tiles, wall ms), its total wall time, and on a third fresh mosaic the per-tile calc_fill_depressions of every tile
(pydem_fill_depressions: device ms summed over the tiles, and wall).  The per-tile fill lets a depression that a seam cuts drain
off the tile; the numbers are what closing the seams costs.  No pass/fail threshold.

The file has three sections: the measurement and (--compiler-report) what hipcc reports for the kernels of
csrc/fill_depressions.hip, each rewritten by its own mode and kept by the other, and notes written by hand, which both keep."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources      # (tools/ is the script directory)

MEASURED, COMPILER, NOTES = '== measurement ==', '== compiler report ==', '== notes =='


def sections(path):
    """{marker: text} of an existing file (a missing section is empty); the notes are written by hand and kept by both modes"""
    text = open(path).read() if os.path.exists(path) else ''
    marks = sorted((text.find(m), m) for m in (MEASURED, COMPILER, NOTES) if text.find(m) >= 0)
    out = {MEASURED: '', COMPILER: '', NOTES: ''}
    for k, (at, m) in enumerate(marks):
        out[m] = text[at + len(m):marks[k + 1][0] if k + 1 < len(marks) else len(text)].strip('\n')
    return out


def write(path, sec):
    with open(path, 'w') as f:
        f.write("Depression filling across tiles (ProcessManager.process_fill_depressions, the pydem_fill_seam_* session of\n"
                "csrc/fill_depressions.hip): cost on the MI355X.  tools/fill_mosaic_cost.py is the measurement.\n")
        for m in (MEASURED, COMPILER, NOTES):
            f.write('\n' + m + '\n' + sec[m] + '\n')


def tile_specs(n, px=30.0, rows=2, cols=4):
    specs = []
    for t in range(rows * cols):
        r, c = t // cols, t % cols
        row0, col0 = r * (n - 1), c * (n - 1)
        specs.append({'shape': (n, n), 'synth': dict(seed=1, row0=row0, col0=col0),
                      'bounds': (col0 * px, -(row0 + n) * px, (col0 + n) * px, -row0 * px)})
    return specs


def mosaic(n):
    from pydem_amd import process_manager
    pm = process_manager.ProcessManager(elev_source_files=tile_specs(n), elev_conditioned=True, devices=[0], out_path='.',
                                        dem_proc_kwargs=dict(fill_flats=False, drain_pits_path=False))
    pm.process_elevation()
    for dp in pm.tiles:
        dp._tile.synchronize()
    return pm


def measure(n):
    warnings.simplefilter('ignore')
    lines = ["2 x 4 tiles of %d^2, one-pixel overlap, one GPU; tiles_in_flight = default" % n]
    for name, eps in (('eps_0', 0.0), ('eps_auto', None)):
        mosaic(n).process_fill_depressions(eps)     # (loads the kernels, sizes the arena and the plane cache)
        pm = mosaic(n)
        t0 = time.perf_counter()
        pm.process_fill_depressions(eps)
        wall = (time.perf_counter() - t0) * 1e3
        lines.append(json.dumps(dict(case=name, what='process_fill_depressions', rounds=pm.fill_rounds, epsilon=pm.fill_depressions_epsilon_used,
                                     wall_ms=round(wall, 3), device_ms=round(sum(r['device_ms'] for r in pm.fill_round_log), 3))))
        for k, r in enumerate(pm.fill_round_log):
            lines.append(json.dumps(dict(case=name, round=k + 1, tiles=r['tiles'], n_lowered=r['n_lowered'], passes=r['passes'],
                                         device_ms=round(r['device_ms'], 3), wall_ms=round(r['wall_ms'], 3))))
        raised = sum(dp.fill_depressions_stats['n_raised'] for dp in pm.tiles)
        pm = mosaic(n)
        t0 = time.perf_counter()
        st = [dp.run_fill_depressions(eps) for dp in pm.tiles]
        wall = (time.perf_counter() - t0) * 1e3
        lines.append(json.dumps(dict(case=name, what='per-tile calc_fill_depressions, summed over the 8 tiles', wall_ms=round(wall, 3),
                                     device_ms=round(sum(s['ms'] for s in st), 3), passes=sum(s['passes'] for s in st),
                                     n_raised=sum(s['n_raised'] for s in st), n_raised_across_tiles=raised)))
        print('\n'.join(l for l in lines if '"%s"' % name in l), flush=True)
    return '\n'.join(lines)


def compiler_report():
    from pydem_amd import build
    rows = kernel_resources('fill_depressions.hip')
    text = ["hipcc %s, -Rpass-analysis=kernel-resource-usage" % ' '.join(build.FLAGS)]
    for name, r in sorted(rows.items()):
        text.append("%-34s %3s VGPRs, scratch %s B/lane, LDS %5s B per workgroup, %s wavefronts per SIMD"
                    % (name, r['vgprs'], r['scratch'], r['lds'], r['occupancy']))
    return '\n'.join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=8192)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fill_mosaic_cost.txt'))
    ap.add_argument('--compiler-report', action='store_true')
    args = ap.parse_args()
    sec = sections(args.out)
    if args.compiler_report:
        sec[COMPILER] = compiler_report()
    else:
        sec[MEASURED] = measure(args.size)
    write(args.out, sec)


if __name__ == '__main__':
    main()
