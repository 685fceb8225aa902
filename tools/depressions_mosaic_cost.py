"""Cost of the depression inventory across tiles (ProcessManager.process_depressions) next to the fill across tiles on the same mosaic.

    python tools/depressions_mosaic_cost.py [--size 8192] [--out profiles/depressions_mosaic_cost.txt]

The mosaic is bench.py's layout, as in tools/fill_mosaic_cost.py: 2 x 4 tiles of --size^2 with a one-pixel overlap, elevations from
the device generator at global mosaic coordinates, all on GPU 0.  One run of each call on a mosaic of its own loads the kernels and
sizes the arena; then, on a fresh mosaic each, process_depressions (rounds of its fill, depressions found, device ms of each part
summed over the tiles, wall ms) and process_fill_depressions(0.0) (rounds, device ms, wall ms).  The inventory runs the same
sessions to the same fixed point and then labels, reduces and writes labels; the ratio says what that costs on top.  No pass/fail
threshold.

The file has two sections: the measurement, rewritten by every run, and notes written by hand, which a run keeps."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MEASURED, NOTES = '== measurement ==', '== notes =='


def sections(path):
    text = open(path).read() if os.path.exists(path) else ''
    out = {MEASURED: '', NOTES: ''}
    a, b = text.find(MEASURED), text.find(NOTES)
    if a >= 0:
        out[MEASURED] = text[a + len(MEASURED):b if b > a else len(text)].strip('\n')
    if b >= 0:
        out[NOTES] = text[b + len(NOTES):].strip('\n')
    return out


def write(path, sec):
    with open(path, 'w') as f:
        f.write("Depression inventory across tiles (ProcessManager.process_depressions, the pydem_fill_seam_label / _inventory / _labels\n"
                "calls of csrc/depressions.hip): cost on the MI355X.  tools/depressions_mosaic_cost.py is the measurement.\n")
        for m in (MEASURED, NOTES):
            f.write('\n' + m + '\n' + sec[m] + '\n')


def measure(n):
    from fill_mosaic_cost import mosaic
    warnings.simplefilter('ignore')
    lines = ["2 x 4 tiles of %d^2, one-pixel overlap, one GPU; tiles_in_flight = default" % n]
    mosaic(n).process_depressions()                 # (loads the kernels, sizes the arena and the plane cache)
    print("warm-up run done", flush=True)
    pm = mosaic(n)
    t0 = time.perf_counter()
    res = pm.process_depressions()
    wall = (time.perf_counter() - t0) * 1e3
    st = pm.depressions_stats
    inv_ms = sum(st['ms'].values())
    lines.append(json.dumps(dict(what='process_depressions', rounds=st['fill_rounds'], n_found=st['n_found'], kept=len(res['table']),
                                 open_sill=int(res['table']['open_sill'].sum()), wall_ms=round(wall, 3), device_ms=round(inv_ms, 3),
                                 device_ms_by_part={k: round(v, 3) for k, v in sorted(st['ms'].items())})))
    del res
    mosaic(n).process_fill_depressions(0.0)
    pm = mosaic(n)
    t0 = time.perf_counter()
    pm.process_fill_depressions(0.0)
    wall = (time.perf_counter() - t0) * 1e3
    fill_ms = sum(r['device_ms'] for r in pm.fill_round_log)
    lines.append(json.dumps(dict(what='process_fill_depressions(0.0)', rounds=pm.fill_rounds, wall_ms=round(wall, 3), device_ms=round(fill_ms, 3))))
    lines.append(json.dumps(dict(what='ratio of device ms, inventory / fill', ratio=round(inv_ms / fill_ms, 3))))
    print('\n'.join(lines), flush=True)
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=8192)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depressions_mosaic_cost.txt'))
    args = ap.parse_args()
    sec = sections(args.out)
    sec[MEASURED] = measure(args.size)
    write(args.out, sec)


if __name__ == '__main__':
    main()
