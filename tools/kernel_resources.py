"""What hipcc reports for the kernels of one unit of pydem_amd/csrc: the one parser of -Rpass-analysis=kernel-resource-usage.

    python tools/kernel_resources.py terrain.hip horizon.hip ... [--csrc DIR]        (no GPU needed)

kernel_resources(unit) compiles the unit alone with build.FLAGS and returns {kernel: {sgprs, vgprs, scratch, occupancy, lds}} of
its own kernels (k_*, in the order of the report; a template's arguments as in the source: k_ta_window<3>, k_fd_relax<true>).
The cost tools put it into their files; the command prints one line per kernel, for comparing two trees (--csrc: the csrc
directory of another checkout)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = {'TotalSGPRs': 'sgprs', 'VGPRs': 'vgprs', 'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'occupancy',
        'LDS Size [bytes/block]': 'lds'}
TYPES = {'d': 'double', 'f': 'float', 'h': 'uint8_t', 'i': 'int', 'y': 'u64'}


def kernel_name(mangled):
    """k_fd_relax_seam<true> from _ZN12_GLOBAL__N_115k_fd_relax_seamILb1EEEv...; a name outside the anonymous namespace as it is"""
    m = re.match(r'_ZN12_GLOBAL__N_1(\d+)', mangled)
    if not m:
        return mangled
    end = m.end() + int(m.group(1))
    name, targs = mangled[m.end():end], re.match(r'I((?:L[bi]\d+E|[dfhiy])+)E', mangled[end:])
    if not targs:
        return name
    args = [TYPES[t] if t else (v if k == 'i' else ('false', 'true')[v != '0']) for k, v, t in re.findall(r'L([bi])(\d+)E|([dfhiy])', targs.group(1))]
    return '%s<%s>' % (name, ', '.join(args))


def kernel_resources(unit, csrc=None):
    from pydem_amd import build
    r = subprocess.run([build.HIPCC] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(csrc or build.CSRC, unit),
                                                      '-o', os.devnull], capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|%s): (\S+)' % '|'.join(re.escape(k) for k in KEYS), line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = kernel_name(m.group(2))
            cur = out.setdefault(name, {}) if name.startswith('k_') else None
        elif cur is not None:
            cur[KEYS[m.group(1)]] = int(m.group(2))
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('units', nargs='+')
    ap.add_argument('--csrc', default=None)
    args = ap.parse_args()
    for unit in args.units:
        for name, r in kernel_resources(unit, args.csrc).items():
            print("%-22s %-26s %3d SGPRs %3d VGPRs scratch %d LDS %5d occupancy %d"
                  % (unit, name, r['sgprs'], r['vgprs'], r['scratch'], r['lds'], r['occupancy']))
