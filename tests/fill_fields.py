"""Designed surfaces for the depression filling (tests/test_fill_depressions_ref.py, tests/test_gpu_fill_depressions.py): small
builders, each returning a float64 elevation (the int16 terraces excepted)."""
import numpy as np


def plane(n, m, z0=500.0, sr=0.5, sc=0.3):
    r, c = np.mgrid[0:n, 0:m]
    return z0 + sr * r + sc * c


BOWL_SHAPE = (96, 80)
BOWL_BOTTOM = (48, 40)
BOWL_RADIUS = 10


def bowl():
    """A tilted plane with a paraboloid bowl of radius 10 cells at the centre: bottom 520, rim 550, above the plane (at most 544
    there).  The bottom is the lowest cell of the bowl, so nothing within 4 cells of it is lower."""
    n, m = BOWL_SHAPE
    z = plane(n, m)
    r, c = np.mgrid[0:n, 0:m]
    d2 = (r - BOWL_BOTTOM[0]) ** 2 + (c - BOWL_BOTTOM[1]) ** 2
    inside = d2 <= BOWL_RADIUS ** 2
    z[inside] = 520.0 + 30.0 * d2[inside] / float(BOWL_RADIUS ** 2)
    return z


def nested():
    """A pit inside a lake inside a larger basin (70, 90): three concentric cones, each with its own sill."""
    n, m = 70, 90
    z = plane(n, m, 300.0, 0.2, 0.1)
    r, c = np.mgrid[0:n, 0:m]
    d = np.hypot(r - 36, c - 47)
    z = np.where(d <= 28, 250.0 + 1.5 * d, z)          # the basin: sill 292 below the plane
    d = np.hypot(r - 33, c - 44)
    z = np.where(d <= 11, 220.0 + 2.0 * d, z)          # the lake in it: sill 242
    d = np.hypot(r - 32, c - 42)
    z = np.where(d <= 3, 200.0 + 4.0 * d, z)           # the pit in the lake: sill 212
    return z


def serpentine_path(n=100, m=100):
    path = [(2, 0), (2, 1)]
    right = True
    for r in range(2, n - 3, 2):
        cols = range(2, m - 2) if right else range(m - 3, 1, -1)
        path += [(r, c) for c in cols]
        if r + 2 < n - 3:
            path.append((r + 1, m - 3 if right else 2))
        right = not right
    return path


def serpentine():
    """A plateau at 1000 with a one-cell channel winding row-wise through it.  The channel descends AWAY from its single outlet
    at the border: the whole channel is one depression that crosses block boundaries dozens of times."""
    z = np.full((100, 100), 1000.0)
    for k, (r, c) in enumerate(serpentine_path()):
        z[r, c] = 900.0 - 0.01 * k
    return z


def corner_spill(k):
    """(64, 64): a basin in one 32 x 32 block whose only spill path is the diagonal step across the corner where the four blocks
    meet -- (31, 31) -> (32, 32) for k = 0, mirrored for k = 1, 2, 3 -- and a diagonal channel from there down to the tile's
    corner.  Every cardinal way out of the basin is the wall (100): the basin fills to the sill at (32, 32), 60, not to 100."""
    z = np.full((64, 64), 100.0)
    z[20:32, 20:32] = 50.0
    z[25, 25] = 40.0
    for i in range(32, 64):
        z[i, i] = 60.0 - (i - 32)
    if k & 1:
        z = z[:, ::-1]
    if k & 2:
        z = z[::-1, :]
    return np.ascontiguousarray(z)


def corner_spill_basin(k):
    """the basin's cells of corner_spill(k)"""
    b = np.zeros((64, 64), bool)
    b[20:32, 20:32] = True
    if k & 1:
        b = b[:, ::-1]
    if k & 2:
        b = b[::-1, :]
    return np.ascontiguousarray(b)


def plateau():
    return np.full((40, 70), 123.0)


def bowl_nan_hole():
    """a no-data hole inside the bowl: its neighbours are open, the bowl only fills up to them"""
    z = bowl()
    z[44:46, 43:45] = np.nan
    return z


def nan_ring(base):
    """a no-data ring enclosing an interior (the interior drains to the ring, the outside to the border and the ring)"""
    z = np.array(base, dtype=np.float64)
    z[20, 15:66] = z[60, 15:66] = np.nan
    z[20:61, 15] = z[20:61, 65] = np.nan
    return z


def all_nan():
    return np.full((40, 40), np.nan)


def negative_zero():
    """negative elevations, and a lake bed of zeros of both signs"""
    z = np.round(bowl() - 535.0)
    r, c = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    z[(z == 0) & ((r + c) % 2 == 0)] = -0.0
    z[30, 30] = -0.0
    return z


def terraces():
    from pydem_amd import synth
    return synth.srtm_int16(96, 80)


def fractal(n, m, nan_rect=False):
    from pydem_amd import synth
    z = synth.fractal(n, m, seed=5)
    if nan_rect:
        z[40:50, 30:45] = np.nan
    return z


def designed():
    """name -> builder of every designed field"""
    d = {'bowl': bowl, 'nested': nested, 'serpentine': serpentine, 'plateau': plateau, 'bowl_nan_hole': bowl_nan_hole,
         'nan_ring': lambda: nan_ring(fractal(96, 80)), 'all_nan': all_nan, 'negative_zero': negative_zero,
         'terraces': lambda: terraces().astype(np.float64)}
    for k in range(4):
        d['corner_spill%d' % k] = (lambda k=k: corner_spill(k))
    return d
