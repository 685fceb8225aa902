"""Build libpydem_hip.so (hipcc, gfx950 only) in-tree: pydem_amd/lib/libpydem_hip.so, and beside it the diagnostic
libpydem_hip_queue.so (the same objects with uca.hip, the per-tile flow accumulation and the only unit that knows the macro, compiled
under -DPYDEM_SWEEP_QUEUE: the frontier-queue sweep schedule that tests/test_gpu_sweep_modes.py checks; it refuses some valid inputs, so
it is never the product library).  The cross-tile edge fix-up, uca_edge.hip, is one object in both.

    python -m pydem_amd.build [--force]

-ffp-contract=off is part of the numerical contract (see csrc/stencil.hip): the facet and
section arithmetic must round like numpy's separate ufunc calls.
"""
import concurrent.futures
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIB = os.path.join(LIBDIR, 'libpydem_hip.so')
SOURCES = ['tile.hip', 'devmem.hip', 'stencil.hip', 'flats.hip', 'uca.hip', 'uca_edge.hip', 'flowdist.hip', 'flowdist_up.hip', 'flowacc_rev.hip', 'flowacc_fwd.hip', 'streamnet.hip', 'flowacc_tree.hip', 'pits.hip', 'synth.hip', 'comm.hip', 'cyutils.hip', 'cond_host.cpp', 'tiff_lzw.cpp', 'cond_device.hip', 'cond_paths.hip', 'fill_depressions.hip', 'depressions.hip', 'hand_table.hip', 'terrain.hip', 'horizon.hip']
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-fno-fast-math',
         '-Wall', '-Wno-unused-function', '-Wno-unused-result']
FLAGS += os.environ.get('PYDEM_HIPCC_FLAGS', '').split()     # kernel-tuning experiments (-D...), not part of the product build
QUEUE_LIB = os.path.join(LIBDIR, 'libpydem_hip_queue.so')
QUEUE_UNIT, QUEUE_FLAGS = 'uca.hip', ['-DPYDEM_SWEEP_QUEUE']


def _deps_mtime():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.h', '.inl'))]
    hdrs.append(os.path.join(HERE, '..', 'include', 'pydem_hip.h'))
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(src, force, extra=(), suffix=''):
    obj = os.path.join(LIBDIR, os.path.splitext(src)[0] + suffix + '.o')
    path = os.path.join(CSRC, src)
    if (not force and os.path.exists(obj)
            and os.path.getmtime(obj) >= max(os.path.getmtime(path), _deps_mtime())):
        return obj, False
    lang = ['-x', 'hip'] if src.endswith('.cpp') else []     # host-only units share internal.h (HIP types): same front end
    subprocess.check_call([HIPCC] + FLAGS + list(extra) + lang + ['-c', path, '-o', obj])
    return obj, True


def _link(lib, objs):
    subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs + ['-L/opt/rocm/lib', '-lrccl'])


def build(force=False, verbose=True):
    os.makedirs(LIBDIR, exist_ok=True)
    jobs = [(s, ()) for s in SOURCES] + [(QUEUE_UNIT, QUEUE_FLAGS)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        res = list(ex.map(lambda j: _compile(j[0], force, j[1], '_queue' if j[1] else ''), jobs))
    objs = [r[0] for r in res[:len(SOURCES)]]
    if force or any(r[1] for r in res[:len(SOURCES)]) or not os.path.exists(LIB):
        _link(LIB, objs)
        if verbose:
            print('built', LIB)
    if force or any(r[1] for r in res) or not os.path.exists(QUEUE_LIB):
        qobj = res[-1][0]
        _link(QUEUE_LIB, [qobj if os.path.basename(o) == os.path.splitext(QUEUE_UNIT)[0] + '.o' else o for o in objs])
        if verbose:
            print('built', QUEUE_LIB)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
