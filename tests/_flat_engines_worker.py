"""Child process of tests/test_gpu_flat_engines.py: the engine thresholds of fill_flats are read once per process, so one
process per setting runs every designed field (tests/flat_fields.py) through DEMProcessor.calc_fill_flats and dumps the
surfaces.  Usage: python _flat_engines_worker.py OUT.npz; the debug lines of the library (PYDEM_COND_DEBUG) go to stderr,
behind a marker line per run."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

RUNS = [(dtype, area) for dtype in ('float64', 'int16') for area in (0.0, None)]      # (None: the default maximum_pit_area)


def run_key(name, dtype, area):
    return '%s/%s/%s' % (name, dtype, 'default' if area is None else 'area%g' % area)


def main(out):
    import flat_fields as F
    from pydem_amd import DEMProcessor
    lib = os.environ.get('PYDEM_TEST_LIB')                 # a scratch build of the library (planted mistakes), never set by the suite
    if lib:
        from pydem_amd import _ffi
        assert _ffi._lib is None
        _ffi.LIB_PATH = lib
    res = {}
    warnings.simplefilter('ignore')
    for f in F.all_fields():
        for dtype, area in RUNS:
            key = run_key(f.name, dtype, area)
            sys.stderr.write("FLATFIELD %s\n" % key)
            sys.stderr.flush()
            kw = {} if area is None else {'maximum_pit_area': area}
            dp = DEMProcessor(elev=f.z.astype(dtype), dX=30.0, dY=30.0, **kw)
            dp.calc_fill_flats()
            assert 'elev' in dp._on_device, key
            res[key] = np.asarray(dp.elev)
            assert res[key].dtype == np.float64, key
    np.savez(out, **res)
    print("FLAT-ENGINES-OK %d" % len(res))


if __name__ == '__main__':
    main(sys.argv[1])
