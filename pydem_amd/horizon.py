"""What the terrain around a cell hides from it, as the mixin `DEMProcessor` inherits: the horizon angle per azimuth, the sky-view
factor, the cast shadow of a given sun and a shaded relief that uses it.  None has a counterpart in the reference class.

`ray_table` builds, on the host, the cells every ray samples and their weights, so that the device and the twin read the same
integers and doubles.  `horizon_ref` is the numpy twin of pydem_horizon (include/pydem_hip.h states the definition): the horizon
tangent is a maximum over a fixed set of products, which no sample order changes, and the sky-view factor is a fixed sequence of
`* + /`, so the device is held to the twin bit for bit.  Nothing in the twin needs a device; the methods of the class have no CPU
fallback.
"""
import collections
import logging
import math

import numpy as np

from . import _ffi
from .terrain import check_z_factor

logger = logging.getLogger(__package__ + '.dem_processing')       # the logger of the class these methods belong to

PLANES = ('svf', 'horizon')
MAX_DIRECTIONS = 64
MAX_STEPS = 1024                # per direction
DEFAULT_CELLS = 100             # max_dist=None: this many times the smaller cell size

RayTable = collections.namedtuple('RayTable', 'start dr dc w azimuths')
RayTable.__doc__ = """The rays of a call.  start: int32 [n_dir + 1], direction d owns the steps start[d] .. start[d + 1] - 1; dr, dc: int16,
the sampled cell's row and column offset; w: float64, z_factor over the distance of that cell's centre; azimuths: float64 [n_dir],
degrees clockwise from north."""


def check_n_dir(n_dir):
    if isinstance(n_dir, (bool, np.bool_)) or not isinstance(n_dir, (int, np.integer)) or not 1 <= int(n_dir) <= MAX_DIRECTIONS:
        raise ValueError("n_dir must be an integer in 1 .. %d (got %r)" % (MAX_DIRECTIONS, n_dir))
    return int(n_dir)


def check_azimuth(azimuth, name='azimuth0'):
    try:
        az = float(azimuth)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number (got %r)" % (name, azimuth))
    if not math.isfinite(az):
        raise ValueError("%s must be finite (got %r)" % (name, azimuth))
    return az


def check_max_dist(max_dist):
    """None, or a finite distance > 0 in ground units"""
    if max_dist is None:
        return None
    try:
        md = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError("max_dist must be None or a number (got %r)" % (max_dist,))
    if not math.isfinite(md) or md <= 0:
        raise ValueError("max_dist must be finite and > 0 (got %r)" % (max_dist,))
    return md


def check_which(which):
    """`which` as a tuple of plane names without repeats, in the caller's order; ValueError for none or an unknown one"""
    if isinstance(which, str):
        which = (which,)
    try:
        names = tuple(which)
    except TypeError:
        raise ValueError("which must be a sequence of plane names (got %r)" % (which,))
    if not names:
        raise ValueError("which is empty: ask for at least one of %s" % (PLANES,))
    bad = [nm for nm in names if not isinstance(nm, str) or nm not in PLANES]
    if bad:
        raise ValueError("unknown horizon planes %r (known: %s)" % (bad, PLANES))
    return tuple(dict.fromkeys(names))


def _ground_direction(azimuth):
    """(sin a, cos a) of an azimuth in degrees, the quadrant taken off first and put back by exact swaps and sign changes, so that
    the direction of azimuth + 90 is the direction of azimuth turned, to the bit; 45 degrees has equal components"""
    a = math.fmod(azimuth, 360.0)
    if a < 0:
        a += 360.0
    q = int(a // 90.0) % 4
    rem = a - 90.0 * q
    if rem == 45.0:
        s = c = math.sqrt(0.5)
    else:
        s, c = math.sin(math.radians(rem)), math.cos(math.radians(rem))
    return ((s, c), (c, -s), (-s, -c), (-c, s))[q]


def _round_half_away(x):
    return np.copysign(np.floor(np.abs(x) + 0.5), x)


def ray_table(n_dir=16, azimuth0=0.0, max_dist=None, gx=1.0, gy=1.0, z_factor=1.0):
    """The ray table of pydem_horizon.  Direction d has the azimuth azimuth0 + d * 360 / n_dir degrees clockwise from north.  Its
    ground direction (sin a, cos a) (east, north) becomes the index-space direction (sc, sr) = (sin a / gx, -cos a / gy) -- rows
    grow to the south, columns to the east --, scaled so that max(|sr|, |sc|) == 1; step k = 1, 2, ... samples the cell
    (round(k * sr), round(k * sc)), halves rounded away from zero, at the distance of that cell's centre,
    sqrt((dc * gx)**2 + (dr * gy)**2); steps are kept while that distance is <= max_dist (ground units; None: 100 * min(gx, gy)),
    and a step weighs z_factor over its distance.  More than 1024 steps in a direction is a ValueError; none (max_dist under a
    cell) is legal."""
    n_dir = check_n_dir(n_dir)
    az0 = check_azimuth(azimuth0)
    md = check_max_dist(max_dist)
    zf = check_z_factor(z_factor)
    gx, gy = float(gx), float(gy)
    if not (math.isfinite(gx) and math.isfinite(gy) and gx > 0 and gy > 0):
        raise ValueError("the cell sizes must be finite and > 0 (got %r, %r)" % (gx, gy))
    if md is None:
        md = DEFAULT_CELLS * min(gx, gy)
    azimuths = np.array([az0 + d * 360.0 / n_dir for d in range(n_dir)], np.float64)
    k = np.arange(1, MAX_STEPS + 2, dtype=np.float64)
    start, drs, dcs, ws = [0], [], [], []
    for a in azimuths:
        east, north = _ground_direction(float(a))
        sc, sr = east / gx, -north / gy
        top = max(abs(sr), abs(sc))
        sr, sc = sr / top, sc / top
        dr, dc = _round_half_away(k * sr), _round_half_away(k * sc)
        dist = np.sqrt((dc * gx) ** 2 + (dr * gy) ** 2)
        beyond = np.nonzero(dist > md)[0]
        if beyond.size == 0:
            raise ValueError("max_dist %r is more than %d steps at azimuth %r: shorten it" % (max_dist, MAX_STEPS, float(a)))
        cnt = int(beyond[0])
        drs.append(dr[:cnt].astype(np.int16))
        dcs.append(dc[:cnt].astype(np.int16))
        ws.append(zf / dist[:cnt])
        start.append(start[-1] + cnt)
    return RayTable(np.array(start, np.int32), np.concatenate(drs), np.concatenate(dcs), np.concatenate(ws).astype(np.float64), azimuths)


def _shifted(n, m, dr, dc):
    """the (destination, source) slices of the cells whose sample (r + dr, c + dc) lies inside an [n, m] tile, or None"""
    r0, r1, c0, c1 = max(0, -dr), min(n, n - dr), max(0, -dc), min(m, m - dc)
    if r0 >= r1 or c0 >= c1:
        return None
    return (slice(r0, r1), slice(c0, c1)), (slice(r0 + dr, r1 + dr), slice(c0 + dc, c1 + dc))


def horizon_ref(elev, table, edge_nan=True, want_horizon=True, want_svf=True):
    """The twin of pydem_horizon: ({'horizon': float64 [n_dir, n, m] tangents, 'svf': float64 [n, m]} as asked for, defined
    cells).  elev: [n, m], NaN = no data; table: a RayTable.  T_d starts at 0.0 and takes every v = (z[sample] - z0) * w that is
    greater (a NaN sample compares false); NaN at a NaN cell and, under edge_nan, where any sample of d falls outside the tile.
    svf = (sum over ascending d, from 0.0, of 1.0 / (1.0 + T_d * T_d)) / n_dir."""
    if np.ma.isMaskedArray(elev):
        elev = np.ma.filled(elev.astype(np.float64), np.nan)
    z = np.asarray(elev, np.float64)
    n, m = z.shape
    n_dir = len(table.start) - 1
    nodata = np.isnan(z)
    hor = np.empty((n_dir, n, m)) if want_horizon else None
    acc = np.zeros((n, m))
    finite = np.ones((n, m), bool)
    rows, cols = np.arange(n)[:, None], np.arange(m)[None, :]
    with np.errstate(all='ignore'):
        for d in range(n_dir):
            T = np.zeros((n, m))
            lo, hi = int(table.start[d]), int(table.start[d + 1])
            for k in range(lo, hi):
                sl = _shifted(n, m, int(table.dr[k]), int(table.dc[k]))
                if sl is None:
                    continue
                dst, src = sl
                v = (z[src] - z[dst]) * table.w[k]
                T[dst] = np.where(v > T[dst], v, T[dst])
            T[nodata] = np.nan
            if edge_nan and hi > lo:
                dr, dc = table.dr[lo:hi].astype(int), table.dc[lo:hi].astype(int)
                complete = (rows + min(dr.min(), 0) >= 0) & (rows + max(dr.max(), 0) < n) & \
                           (cols + min(dc.min(), 0) >= 0) & (cols + max(dc.max(), 0) < m)
                T[~complete] = np.nan
            if want_horizon:
                hor[d] = T
            acc = acc + 1.0 / (1.0 + T * T)
            finite &= np.isfinite(T)
        svf = acc / float(n_dir)
    out = {}
    if want_horizon:
        out['horizon'] = hor
    if want_svf:
        out['svf'] = svf
    return out, int(np.isfinite(svf).sum()) if want_svf else int(finite.sum())


def shadow_of(T, altitude):
    """1.0 where the horizon tangent T leaves a sun at `altitude` degrees visible (T <= tan(altitude)), 0.0 where it hides it,
    NaN where T is NaN.  The tangent of the altitude is computed once."""
    limit = math.tan(math.radians(altitude))
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(T), np.nan, np.where(T <= limit, 1.0, 0.0))


def cast_shadow_ref(elev, azimuth, altitude, max_dist=None, gx=1.0, gy=1.0, z_factor=1.0, edge_nan=True):
    """The twin of calc_cast_shadow: one direction of horizon_ref at the sun's azimuth, then shadow_of."""
    table = ray_table(1, azimuth, max_dist, gx, gy, z_factor)
    out, _ = horizon_ref(elev, table, edge_nan, True, False)
    return shadow_of(out['horizon'][0], check_altitude(altitude))


def check_altitude(altitude):
    try:
        alt = float(altitude)
    except (TypeError, ValueError):
        raise ValueError("altitude must be a number (got %r)" % (altitude,))
    if not (0 < alt <= 90):
        raise ValueError("altitude must be in (0, 90] degrees (got %r)" % (altitude,))
    return alt


class HorizonAnalyses(object):
    """The horizon methods of DEMProcessor and their result attributes."""

    horizon = None              # {'svf', 'horizon', 'azimuths'} of the last calc_horizon
    horizon_stats = None        # {'ms', 'n_defined', 'n_dir', 'steps'} of the last calc_horizon

    def _horizon_cell_size(self):
        """one cell size for the whole call: dX2 / dY2 of the tile's middle row"""
        mid = int(self.shape[0]) // 2
        return float(np.asarray(self.dX2, np.float64)[mid]), float(np.asarray(self.dY2, np.float64)[mid])

    def calc_horizon(self, n_dir=16, max_dist=None, azimuth0=0.0, z_factor=1.0, edge_nan=True, which=('svf',)):
        """The horizon around every cell: for `n_dir` (1 .. 64) azimuths azimuth0 + d * 360 / n_dir degrees clockwise from north,
        the tangent of the highest elevation angle under which a cell within `max_dist` (ground units; None: 100 times the
        smaller cell size; at most 1024 cells) stands above the cell, never below the horizontal (0), with elevations stretched by
        `z_factor`; and the sky-view factor, the mean over the azimuths of cos^2 of that angle (1: open sky).  include/pydem_hip.h
        (pydem_horizon) and `ray_table` state the definition: nearest-cell samples along each ray, no data does not obstruct.
        which: any of 'svf' ([n, m]) and 'horizon' ([n_dir, n, m] tangents; 8 n m bytes per direction, on the host and on the
        device).  The cell size is ONE pair for the whole call, dX2 / dY2 of the tile's middle row n // 2: exact on projected
        tiles, an approximation on geographic ones.  With edge_nan a direction is NaN where its ray leaves the tile, so that a
        finite value is a complete one; without, samples off the tile are skipped.  Works on the tile's current elevation --
        conditioned if conditioning has run --, needs no slopes or flow graph and changes no other result.  Returns the dict of the
        planes asked for and 'azimuths' (degrees), kept as `horizon`; `horizon_stats` holds the device ms, the defined cells, the
        directions and the steps of all rays.  Per tile: a ray ends at the tile's border."""
        names = check_which(which)
        n_dir = check_n_dir(n_dir)
        az0 = check_azimuth(azimuth0)
        md = check_max_dist(max_dist)
        zf = check_z_factor(z_factor)
        shape = tuple(self.shape)
        if min(shape) < 3:
            # (the library holds no tile under 3 x 3: all NaN without a launch, as calc_terrain_attributes answers it)
            if _ffi.device_count() < 1:
                raise _ffi.HipError("no HIP device is visible (there is no CPU fallback)")
            azimuths = np.array([az0 + d * 360.0 / n_dir for d in range(n_dir)], np.float64)
            planes = {nm: np.full(shape if nm == 'svf' else (n_dir,) + shape, np.nan) for nm in names}
            ms, count, steps = 0.0, 0, 0
        else:
            gx, gy = self._horizon_cell_size()
            table = ray_table(n_dir, az0, md, gx, gy, zf)
            azimuths, steps = table.azimuths, int(table.start[-1])
            tile = self._ensure_tile()
            self._push('elev')
            logger.info("Starting horizon (%d directions, %d steps)" % (n_dir, steps))
            planes, ms, count = tile.horizon(table, bool(edge_nan), 'horizon' in names, 'svf' in names)
        out = {nm: planes[nm] for nm in names}
        out['azimuths'] = azimuths
        self.horizon = out
        self.horizon_stats = dict(ms=ms, n_defined=count, n_dir=n_dir, steps=steps)
        return out

    def calc_sky_view_factor(self, n_dir=16, max_dist=None, z_factor=1.0, edge_nan=True):
        """The 'svf' plane of calc_horizon: the fraction of the sky a cell sees, 0 .. 1."""
        return self.calc_horizon(n_dir, max_dist, 0.0, z_factor, edge_nan, ('svf',))['svf']

    def calc_cast_shadow(self, azimuth, altitude, max_dist=None, z_factor=1.0, edge_nan=True):
        """The cast shadow of a sun at `azimuth` degrees clockwise from north and `altitude` degrees above the horizon (in
        (0, 90]): 1.0 where the cell is lit -- the horizon tangent of that one direction is <= tan(altitude) --, 0.0 where
        the terrain within `max_dist` hides the sun, NaN where the tangent is NaN (no data; under edge_nan, where the ray leaves
        the tile).  One direction of calc_horizon; the comparison is on the host."""
        az = check_azimuth(azimuth, 'azimuth')
        alt = check_altitude(altitude)
        T = self.calc_horizon(1, max_dist, az, z_factor, edge_nan, ('horizon',))['horizon'][0]
        return shadow_of(T, alt)

    def calc_shaded_relief(self, azimuth=315.0, altitude=45.0, z_factor=1.0, window=3, max_dist=None):
        """calc_hillshade(azimuth, altitude, z_factor, window) times calc_cast_shadow(azimuth, altitude, max_dist, z_factor,
        edge_nan=False): a hillshade that knows the ridge between the cell and the sun."""
        az = check_azimuth(azimuth, 'azimuth')
        alt = check_altitude(altitude)
        check_max_dist(max_dist)
        shade = self.calc_hillshade(az, alt, z_factor, window)
        return shade * self.calc_cast_shadow(az, alt, max_dist, z_factor, edge_nan=False)
