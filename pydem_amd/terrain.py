"""Terrain attributes at a chosen scale, as the mixin `DEMProcessor` inherits: gradient, aspect, profile / plan / tangential /
mean curvature and hillshade from a least-squares quadratic over a (2k+1)^2 window (Evans 1980 at k = 1, Wood 1996 above).  None
has a counterpart in the reference class.

`terrain_attributes_ref` is the numpy twin of pydem_terrain_attributes (include/pydem_hip.h states the definition): shifted-plane
additions in the operand order of the header, so that the device is held to it bit for bit (the aspect, which passes through
atan2, to a few ulp).  Nothing in the twin needs a device; the methods of the class have no CPU fallback.
"""
import logging
import math

import numpy as np

from . import _ffi

logger = logging.getLogger(__package__ + '.dem_processing')       # the logger of the class these methods belong to

ATTRIBUTES = _ffi.Tile.TERRAIN_ATTRS
CURVATURES = ('profile', 'plan', 'tangential', 'mean')
DEFAULT_ATTRIBUTES = ('gradient', 'aspect', 'profile', 'plan', 'tangential', 'mean')
MIN_WINDOW, MAX_WINDOW = 3, 15
TWO_PI = 6.283185307179586


def check_window(window):
    """`window` as its half width k; ValueError unless it is an odd integer in 3 .. 15"""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)):
        raise ValueError("window must be an odd integer in %d .. %d (got %r)" % (MIN_WINDOW, MAX_WINDOW, window))
    w = int(window)
    if w < MIN_WINDOW or w > MAX_WINDOW or w % 2 == 0:
        raise ValueError("window must be an odd integer in %d .. %d (got %r)" % (MIN_WINDOW, MAX_WINDOW, window))
    return w // 2


def check_which(which):
    """`which` as a tuple of attribute names without repeats, in the caller's order; ValueError for none or an unknown one"""
    if isinstance(which, str):
        which = (which,)
    try:
        names = tuple(which)
    except TypeError:
        raise ValueError("which must be a sequence of attribute names (got %r)" % (which,))
    if not names:
        raise ValueError("which is empty: ask for at least one of %s" % (ATTRIBUTES,))
    bad = [nm for nm in names if not isinstance(nm, str) or nm not in ATTRIBUTES]
    if bad:
        raise ValueError("unknown terrain attributes %r (known: %s)" % (bad, ATTRIBUTES))
    return tuple(dict.fromkeys(names))


def check_z_factor(z_factor):
    try:
        zf = float(z_factor)
    except (TypeError, ValueError):
        raise ValueError("z_factor must be a number (got %r)" % (z_factor,))
    if not math.isfinite(zf) or zf <= 0:
        raise ValueError("z_factor must be finite and > 0 (got %r)" % (z_factor,))
    return zf


def light_vector(azimuth, altitude):
    """The unit vector to the sun (Le, Ln, Lu: east, north, up) of an azimuth (degrees clockwise from north) and an altitude
    (degrees above the horizon, in (0, 90]); ValueError otherwise.  Computed once: the device and the twin get the same doubles."""
    try:
        az, alt = float(azimuth), float(altitude)
    except (TypeError, ValueError):
        raise ValueError("azimuth and altitude must be numbers (got %r, %r)" % (azimuth, altitude))
    if not math.isfinite(az):
        raise ValueError("azimuth must be finite (got %r)" % (azimuth,))
    if not (0 < alt <= 90):
        raise ValueError("altitude must be in (0, 90] degrees (got %r)" % (altitude,))
    az, alt = math.radians(az), math.radians(alt)
    return (math.sin(az) * math.cos(alt), math.cos(az) * math.cos(alt), math.sin(alt))


def fit_constants(k):
    """(N, S2, D1, D2, D11) of the half width k: exact integers held as doubles"""
    N = 2 * k + 1
    S2 = k * (k + 1) * N // 3
    S4 = k * (k + 1) * N * (3 * k * k + 3 * k - 1) // 15
    return float(N), float(S2), float(N * S2), float(N * S4 - S2 * S2), float(S2 * S2)


def terrain_attributes_ref(elev, dX2, dY2, window=3, which=DEFAULT_ATTRIBUTES, light=None, z_factor=1.0):
    """The twin of pydem_terrain_attributes: ({name: float64 [n, m]}, defined cells).  elev: [n, m], NaN = no data; dX2, dY2: [n]
    cell sizes per row; light: (Le, Ln, Lu), needed for 'hillshade'.  Every plane is NaN where the window leaves the tile or its
    sum M00 is NaN (a NaN elevation in it); a tile smaller than the window is all NaN."""
    k = check_window(window)
    names = check_which(which)
    zf = check_z_factor(z_factor)
    if 'hillshade' in names and light is None:
        raise ValueError("a hillshade needs the light vector")
    if np.ma.isMaskedArray(elev):
        elev = np.ma.filled(elev.astype(np.float64), np.nan)
    z = np.asarray(elev, np.float64)
    n, m = z.shape
    out = {nm: np.full((n, m), np.nan) for nm in names}
    ni, mi = n - 2 * k, m - 2 * k
    if ni <= 0 or mi <= 0:
        return out, 0
    N, S2, D1, D2, D11 = fit_constants(k)
    gx = np.asarray(dX2, np.float64)[k:n - k, None]
    gy = np.asarray(dY2, np.float64)[k:n - k, None]
    with np.errstate(all='ignore'):
        # row moments of every row, over the interior columns: each from 0.0, ascending i
        R0, R1, R2 = (np.zeros((n, mi)) for _ in range(3))
        for i in range(-k, k + 1):
            Z = z[:, k + i:m - k + i]
            R0 = R0 + Z
            R1 = R1 + float(i) * Z
            R2 = R2 + float(i * i) * Z
        # window moments: each from 0.0, ascending j
        M00, M10, M20, M01, M02, M11 = (np.zeros((ni, mi)) for _ in range(6))
        for j in range(-k, k + 1):
            r0, r1, r2 = R0[k + j:n - k + j], R1[k + j:n - k + j], R2[k + j:n - k + j]
            M00 = M00 + r0
            M10 = M10 + r1
            M20 = M20 + r2
            M01 = M01 + float(j) * r0
            M02 = M02 + float(j * j) * r0
            M11 = M11 + float(j) * r1
        defined = ~np.isnan(M00)
        d = M10 / D1
        e = M01 / D1
        cxy = M11 / D11
        h = (S2 * M00) / N
        a = (M20 - h) / D2
        b = (M02 - h) / D2
        p = d / gx
        q = -(e / gy)
        r = (2.0 * a) / (gx * gx)
        t = (2.0 * b) / (gy * gy)
        s = -(cxy / (gx * gy))
        g2 = p * p + q * q
        flat = g2 == 0.0
        w = 1.0 + g2
        pq2 = 2.0 * (p * q)
        sw = np.sqrt(w)
        planes = {}
        if 'dzdx' in names:
            planes['dzdx'] = p
        if 'dzdy' in names:
            planes['dzdy'] = q
        if 'gradient' in names:
            planes['gradient'] = np.sqrt(g2)
        if 'aspect' in names:
            v = np.arctan2(-p, -q)
            v = np.where(v < 0.0, v + TWO_PI, v)
            planes['aspect'] = np.where(flat, -1.0, v)
        if 'profile' in names:
            A = ((p * p) * r + pq2 * s) + (q * q) * t
            planes['profile'] = np.where(flat, 0.0, -A / (g2 * (w * sw)))
        if 'plan' in names or 'tangential' in names:
            B = ((q * q) * r - pq2 * s) + (p * p) * t
            if 'plan' in names:
                planes['plan'] = np.where(flat, 0.0, -B / (g2 * np.sqrt(g2)))
            if 'tangential' in names:
                planes['tangential'] = np.where(flat, 0.0, -B / (g2 * sw))
        if 'mean' in names:
            C = ((1.0 + q * q) * r - pq2 * s) + (1.0 + p * p) * t
            planes['mean'] = -C / (2.0 * (w * sw))
        if 'hillshade' in names:
            Le, Ln, Lu = (float(v) for v in light)
            zp, zq = zf * p, zf * q
            v = ((Lu - zp * Le) - zq * Ln) / np.sqrt(1.0 + (zp * zp + zq * zq))
            planes['hillshade'] = np.where(v > 0.0, v, 0.0)
    for nm in names:
        out[nm][k:n - k, k:m - k] = np.where(defined, planes[nm], np.nan)
    return out, int(defined.sum())


class TerrainAnalyses(object):
    """The terrain-attribute methods of DEMProcessor and their result attributes."""

    terrain_attributes = None           # {name: float64 array} of the last calc_terrain_attributes
    terrain_attributes_stats = None     # {'ms', 'n_defined', 'window'} of the last calc_terrain_attributes

    def calc_terrain_attributes(self, which=DEFAULT_ATTRIBUTES, window=3, azimuth=315.0, altitude=45.0, z_factor=1.0):
        """Terrain attributes at the scale of a `window` x `window` least-squares quadratic (odd, 3 .. 15; Evans 1980 at 3, Wood
        1996 above): any of 'dzdx', 'dzdy' (the gradient's components, x east, y north), 'gradient' (rise over run, the unit of
        `mag`), 'aspect' (azimuth of the downslope direction, radians clockwise from north, -1 on flats), 'profile', 'plan',
        'tangential', 'mean' (curvatures, positive = convex after Florinsky / Shary) and 'hillshade' (0 .. 1, the sun at `azimuth`
        degrees clockwise from north and `altitude` degrees above the horizon, elevations stretched by `z_factor`).
        include/pydem_hip.h (pydem_terrain_attributes) states every formula.  Works on the tile's current elevation --
        conditioned if conditioning has run -- before calc_slopes_directions as well as after it, and changes no other result.
        A cell nearer than window // 2 cells to the border, or with a no-data cell in its window, is NaN.  Returns {name: float64
        array}, kept as `terrain_attributes`; `terrain_attributes_stats` holds the device ms, the defined cells and the window.
        Per tile."""
        names = check_which(which)
        k = check_window(window)
        zf = check_z_factor(z_factor)
        light = light_vector(azimuth, altitude)
        shape = tuple(self.shape)
        if min(shape) < 3:
            # (the library holds no tile under 3 x 3; such a tile is smaller than every window: all NaN by definition, no launch)
            if _ffi.device_count() < 1:
                raise _ffi.HipError("no HIP device is visible (there is no CPU fallback)")
            planes, ms, count = {nm: np.full(shape, np.nan) for nm in names}, 0.0, 0
        else:
            tile = self._ensure_tile()
            self._push('elev')
            logger.info("Starting terrain attributes (window %d)" % (2 * k + 1))
            planes, ms, count = tile.terrain_attributes(names, k, light, zf)
        self.terrain_attributes = planes
        self.terrain_attributes_stats = dict(ms=ms, n_defined=count, window=2 * k + 1)
        return planes

    def calc_curvature(self, kind='profile', window=3):
        """One curvature plane of calc_terrain_attributes: 'profile', 'plan', 'tangential' or 'mean'."""
        if not isinstance(kind, str) or kind not in CURVATURES:
            raise ValueError("kind must be one of %s (got %r)" % (CURVATURES, kind))
        return self.calc_terrain_attributes((kind,), window)[kind]

    def calc_hillshade(self, azimuth=315.0, altitude=45.0, z_factor=1.0, window=3):
        """The hillshade plane of calc_terrain_attributes."""
        return self.calc_terrain_attributes(('hillshade',), window, azimuth, altitude, z_factor)['hillshade']
