"""What the GPU tests of the flow-graph analyses share (test_gpu_weighted_uca, _dist_down, _dist_up, _rev_accum, _fwd_accum,
_stream_network, _tree_accum, _flow_fields, _flowgraph_bits): the (oracle, device processor) pairs they run on, the child
process of the schedule tests, the snapshot of a tile's state, and the comparators.  A plain module: no tests, no marks; the
device is touched only by the builders that are called."""
import functools
import hashlib
import os
import subprocess
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the pairs: (oracle after calc_uca, device processor after calc_uca)
def pair(z, drain_pits=True, **spacing):
    """... on the elevation z"""
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    o = O.OracleDEM(z, drain_pits=drain_pits, **spacing)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
        dp = DEMProcessor(elev=z, fill_flats=False, drain_pits_path=False, drain_pits=drain_pits, **spacing)
        dp.calc_slopes_directions()
        dp.calc_uca()
    return o, dp


def fractal_pair(shape, seed):
    """... on a synthetic tile, drain_pits=True: a pair of the caller's own"""
    from pydem_amd import synth
    return pair(synth.fractal(shape[0], shape[1], seed=seed, top_shift=7, n_octaves=7), dX=30.0, dY=30.0)


shared_fractal_pair = functools.lru_cache(maxsize=None)(fractal_pair)      # one per (shape, seed) and process: for calls that leave the tile as it was


def deep_pair(shape=(900, 600)):
    """... on a ramp as long as the tile: the depth of the flow graph is the tile's length, not a hillslope's"""
    n, m = shape
    row, col = np.arange(n, dtype=np.float64)[:, None], np.arange(m, dtype=np.float64)[None, :]
    z = 2000 - 1.5 * row + 10 * np.sin(col / 37) * row / n + np.random.default_rng(1).normal(0, 0.4, (n, m))
    return pair(z, dX=30.0, dY=30.0)


shared_deep_pair = functools.lru_cache(maxsize=None)(deep_pair)


def nan_speck_pair(shape, specks, fixed):
    """(elevation, oracle, device processor, the generator that placed the specks) of a fractal tile with `specks` random
    no-data cells and the `fixed` ones, which lie on the tile's border"""
    from pydem_amd import synth
    n, m = shape
    z = synth.fractal(n, m, seed=7, top_shift=7, n_octaves=7)
    rng = np.random.default_rng(3)
    z[rng.integers(0, n, specks), rng.integers(0, m, specks)] = np.nan
    for cell in fixed:
        z[cell] = np.nan
    o, dp = pair(z, dX=30.0, dY=30.0)
    return z, o, dp, rng


def circular_case(loop):
    """The hand-made loop fields of test_gpu_parity.py (oracle after calc_uca, device processor after calc_uca)."""
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    n, m = 9, 10
    elev = np.full((n, m), 10.0)
    direction = np.full((n, m), 1.5 * np.pi)
    E, N, W, S = 0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi
    if loop == 'two_cells':
        direction[3, 3] = E; direction[3, 4] = W
    elif loop == 'three_cells':
        direction[3, 3] = E; direction[3, 4] = S; direction[4, 4] = 0.75 * np.pi
    else:
        direction[2, 2] = E; direction[2, 3] = W
        direction[5, 6] = S; direction[6, 6] = N
    mag = np.ones((n, m))
    flats = np.zeros((n, m), bool)
    o = O.OracleDEM(elev, dX=2.0, dY=3.0)
    o.mag, o.direction, o.flats = mag.copy(), direction.copy(), flats.astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
        dp = DEMProcessor(elev=elev, dX=2.0, dY=3.0, mag=mag.copy(), direction=direction.copy(), flats=flats.copy(),
                          fill_flats=False, drain_pits_path=False)
        dp.calc_uca()
    assert o.stats[0] > 1, "the case is meant to need the re-seed loop"
    return o, dp


def random_weights(shape, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 2.0, shape)
    w[rng.random(shape) < 0.15] = 0.0                                # >= 10 % exact zeros
    assert (w == 0).mean() >= 0.10
    return w


def _strips(n, m, seed):
    """random edge_init_data [data, done, todo] for an edge round of an n x m tile"""
    rng = np.random.default_rng(seed)
    lens = dict(left=n, right=n, top=m, bottom=m)
    data = {k: rng.uniform(0, 5000, v) for k, v in lens.items()}
    done = {k: rng.random(v) < 0.5 for k, v in lens.items()}
    todo = {k: rng.random(v) < 0.3 for k, v in lens.items()}
    return [data, done, todo]


# ---- a child process, for switches that are read once per process
def run_child(body, env=None, timeout=600):
    """A python child with the GPU open (one at a time): `body` runs after `from flowgraph_kit import *` and imports what it
    needs of the calling test's module itself; it must print CHILD-OK."""
    script = "\n".join(["import sys, warnings", "sys.path.insert(0, %r); sys.path.insert(0, %r)" % (ROOT, HERE),
                        "warnings.simplefilter('ignore')", "import numpy as np",
                        "from flowgraph_kit import *", body])
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, '-c', script], env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0 and 'CHILD-OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


# ---- the state a call must leave alone
def _held_fields(dp):
    """every field of the tile that can be downloaded, by field id"""
    from pydem_amd import _ffi
    out = {}
    for f in range(12):
        try:
            out[f] = dp._tile.download(f)
        except _ffi.HipError:
            pass
    return out


def _snapshot(dp):
    return _held_fields(dp), dp._tile.graph_words(), dp._tile.pit_edges(), dp.timings


def _same_snapshot(a, b):
    fa, ga, pa, ta = a
    fb, gb, pb, tb = b
    assert sorted(fa) == sorted(fb)
    for f in fa:
        assert fa[f].tobytes() == fb[f].tobytes(), "field %d changed" % f
    assert np.array_equal(ga, gb)
    for x, y in zip(pa, pb):
        assert x.tobytes() == y.tobytes()
    assert ta == tb, [(k, ta[k], tb[k]) for k in ta if ta[k] != tb[k]]


# ---- comparators
def bits(a):
    """sha256 of the float64 bytes: what the schedule tests ship across processes"""
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def assert_same_bits(dev, ref, what):
    """identical NaN patterns, and identical bit patterns of every other cell (-0.0 is not 0.0)"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    nd, nr = np.isnan(dev), np.isnan(ref)
    assert np.array_equal(nd, nr), "%s: NaN patterns differ (%d device, %d reference)" % (what, nd.sum(), nr.sum())
    bad = dev[~nd].view(np.int64) != ref[~nr].view(np.int64)
    assert not bad.any(), "%s: %d cells differ in their bits" % (what, bad.sum())


def assert_bound(dev, ref, refabs, what, bound, floor=0.0):
    """identical NaN patterns, and |dev - ref| <= bound * |refabs| + floor cell by cell; prints the worst ratio"""
    dev, ref, refabs = (np.asarray(x, np.float64) for x in (dev, ref, refabs))
    nd, nr = np.isnan(dev), np.isnan(ref)
    assert np.array_equal(nd, nr), "%s: NaN patterns differ (%d device, %d reference)" % (what, nd.sum(), nr.sum())
    err = np.abs(dev[~nr] - ref[~nr])
    scale = np.abs(refabs[~nr])
    lim = bound * scale + floor
    with np.errstate(invalid='ignore'):
        worst = float(np.nanmax(np.r_[0.0, err / np.maximum(scale, 1e-300)]))
    print("%s: %.1f %% NaN, worst |dev - ref| / refabs %.3g" % (what, 100 * nr.mean(), worst))
    assert (err <= lim).all(), "%s: %d cells off, worst %.3g of the scale (bound %.3g)" % (what, (err > lim).sum(), worst, bound)
