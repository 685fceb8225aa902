"""The host side of DEMProcessor.calc_hand_hydraulics and calc_inundation: the numpy twin of pydem_hand_table
(include/pydem_hip.h states every rule), the hydraulic table and the synthetic rating curve made from its integers, the stage
of a discharge and the inundation depth.  Plain numpy on planes: nothing here needs a device."""
import warnings

import numpy as np

from .conditioning import fixed_point

MAX_STAGES = 1024
# the four words of a (zone, bin) of the table
CELLS, AREA, MOMENT, BED = 0, 1, 2, 3
TABLE_COLUMNS = ('cells', 'area', 'volume', 'bed_area', 'top_width', 'xs_area', 'wetted_perimeter', 'hydraulic_radius', 'discharge')


def check_stages(stages):
    """`stages` as a float64 vector: 1 .. MAX_STAGES values, finite, strictly ascending; ValueError otherwise"""
    try:
        st = np.array(stages, dtype=np.float64, ndmin=1)
    except (TypeError, ValueError):
        raise ValueError("stages must be a sequence of numbers (got %r)" % (stages,))
    if st.ndim != 1 or not (1 <= st.size <= MAX_STAGES):
        raise ValueError("stages must be a vector of 1 .. %d values (got shape %r)" % (MAX_STAGES, st.shape))
    if not np.isfinite(st).all():
        raise ValueError("stages must be finite")
    if not (np.diff(st) > 0).all():
        raise ValueError("stages must be strictly ascending")
    return np.ascontiguousarray(st)


def hand_table_ref(zone, hand, stages, dX2, dY2, mag, K):
    """The twin of pydem_hand_table: (int64 [K, S, 4], int64 [K, 2], (q_area, q_moment, q_bed)) -- per zone 1..K and bin (the
    number of stages < h: searchsorted 'left') the cells and the fixed-point sums of a = dX2[r] * dY2[r], a * h and
    a * sqrt(1 + mag * mag) (a non-finite mag counts as slope 0); per zone the NaN cells and the cells above the top stage.
    zone < 1 is skipped; ValueError for a zone > K, bad stages and a term that is not finite (h = -inf)."""
    st = check_stages(stages)
    S, K = st.size, int(K)
    zone = np.asarray(zone)
    n, m = zone.shape
    hf = np.asarray(hand, np.float64).reshape(-1)
    mf = np.asarray(mag, np.float64).reshape(-1)
    if K < 0 or hf.size != n * m or mf.size != n * m:
        raise ValueError("hand_table_ref: K = %d, planes of %d / %d cells for zones of shape %r" % (K, hf.size, mf.size, zone.shape))
    zf = zone.reshape(-1).astype(np.int64)
    if zf.size and zf.max() > K:
        raise ValueError("the zone plane holds the id %d, above the %d zones of the call" % (int(zf.max()), K))
    row_area = np.asarray(dX2, np.float64) * np.asarray(dY2, np.float64)
    inside = zf >= 1
    is_nan = np.isnan(hf)
    with np.errstate(invalid='ignore'):
        above = hf > st[-1]
    skipped = np.zeros((K, 2), np.int64)
    skipped[:, 0] = np.bincount(zf[inside & is_nan] - 1, minlength=K)[:K]
    skipped[:, 1] = np.bincount(zf[inside & above] - 1, minlength=K)[:K]
    c = np.flatnonzero(inside & ~is_nan & ~above)
    a, h, mg = row_area[c // m], hf[c], mf[c]
    with np.errstate(invalid='ignore', over='ignore'):
        pm = a * h
        pb = a * np.where(np.isfinite(mg), np.sqrt(1.0 + mg * mg), 1.0)
    terms = (a, pm, pb)
    largest = [float(np.abs(p).max()) if p.size else 0.0 for p in terms]
    if not np.isfinite(largest).all():
        raise ValueError("a term of the sums is not finite (-inf in the HAND plane, a slope or a spacing out of range)")
    key = (zf[c] - 1) * S + np.searchsorted(st, h, side='left')
    ints = np.zeros((K * S, 4), np.int64)
    ints[:, CELLS] = np.bincount(key, minlength=K * S)[:K * S]
    quanta = []
    for col, p, big in zip((AREA, MOMENT, BED), terms, largest):
        shift, q = fixed_point(n * m, big)
        np.add.at(ints[:, col], key, np.rint(np.ldexp(p, shift)).astype(np.int64))
        quanta.append(q)
    return ints.reshape(K, S, 4), skipped, tuple(quanta)


def hydraulic_table(ints, quanta, stages, length, slope, manning_n):
    """The hydraulic table of the integers of pydem_hand_table: {column: (K, S) array} with, from the int64 sums cumulated over
    the bins (cumN, cumA, cumM, cumB at stage j: everything with HAND <= stages[j]),
        cells = cumN;  area = cumA * q_a;  volume = stages[j] * area - cumM * q_m;  bed_area = cumB * q_b;
        top_width = area / length;  xs_area = volume / length;  wetted_perimeter = bed_area / length;
        hydraulic_radius = volume / bed_area;
        discharge = xs_area * hydraulic_radius ** (2/3) * sqrt(slope) / manning_n   (Manning),
    discharge NaN where slope is not > 0, length is not > 0 or bed_area is 0.  length, slope: (K,) per zone."""
    ints = np.asarray(ints, np.int64)
    st = np.asarray(stages, np.float64)
    K, S = ints.shape[0], ints.shape[1]
    length = np.asarray(length, np.float64).reshape(K)
    slope = np.asarray(slope, np.float64).reshape(K)
    cum = np.cumsum(ints, axis=1, dtype=np.int64)
    q_a, q_m, q_b = quanta
    out = {}
    out['cells'] = cum[:, :, CELLS].copy()
    area = cum[:, :, AREA] * q_a
    volume = st[None, :] * area - cum[:, :, MOMENT] * q_m
    bed = cum[:, :, BED] * q_b
    L = length[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        out['area'], out['volume'], out['bed_area'] = area, volume, bed
        out['top_width'] = area / L
        out['xs_area'] = volume / L
        out['wetted_perimeter'] = bed / L
        radius = volume / bed
        out['hydraulic_radius'] = radius
        ok = (slope > 0)[:, None] & (L > 0) & (bed != 0)
        flow = out['xs_area'] * radius ** (2.0 / 3.0) * np.sqrt(np.where(slope > 0, slope, np.nan))[:, None] / float(manning_n)
        out['discharge'] = np.where(ok, flow, np.nan)
    return out


class HandHydraulics(object):
    """The result of calc_hand_hydraulics.  stages: (S,); link_ids, length, slope, cells_nan, cells_above: (K,), one entry per link
    of the stream network, in the order of its table; cells, area, volume, bed_area, top_width, xs_area, wetted_perimeter,
    hydraulic_radius, discharge: (K, S), the state of each link's catchment with the water at stages[j] above its drainage.
    ints, skipped, quanta: what pydem_hand_table returned; zone: the basin plane the table was reduced over (None for a table
    made by hand); hand: the HAND plane, once calc_inundation has needed it."""

    def __init__(self, stages, link_ids, table, cells_nan, cells_above, length, slope, ints=None, skipped=None, quanta=None, zone=None,
                 manning_n=None):
        self.stages = np.asarray(stages, np.float64)
        self.link_ids = np.asarray(link_ids)
        for k in TABLE_COLUMNS:
            setattr(self, k, table[k])
        self.cells_nan, self.cells_above = np.asarray(cells_nan), np.asarray(cells_above)
        self.length, self.slope = np.asarray(length, np.float64), np.asarray(slope, np.float64)
        self.ints, self.skipped, self.quanta, self.zone, self.manning_n = ints, skipped, quanta, zone, manning_n
        self.hand = None
        self.stream_set = None          # (mask, uca_threshold) of the call that made the table: calc_inundation's HAND uses it

    def __repr__(self):
        return "HandHydraulics(%d links, %d stages)" % (self.link_ids.size, self.stages.size)


def stage_for_discharge(stages, rating, discharge):
    """The stage of a discharge per link, read off its rating curve.  rating: (K, S) discharges at `stages`; discharge: (K,).
    Per link, np.interp over its finite rating points: below the first point the first stage, above the last NaN; NaN for a
    link without a finite point or with a NaN discharge, and NaN with a warning for a rating that is not non-decreasing."""
    st = np.asarray(stages, np.float64)
    rating = np.asarray(rating, np.float64)
    q = np.asarray(discharge, np.float64)
    K = rating.shape[0]
    out = np.full(K, np.nan)
    bad = 0
    for k in range(K):
        ok = np.isfinite(rating[k])
        if not ok.any() or np.isnan(q[k]):
            continue
        xp, fp = rating[k][ok], st[ok]
        if (np.diff(xp) < 0).any():
            bad += 1
            continue
        out[k] = np.interp(q[k], xp, fp, right=np.nan)
    if bad:
        warnings.warn("%d links have a rating curve that is not non-decreasing: their stage is NaN" % bad)
    return out


def inundation_depth(hand, zone, stage):
    """max(stage[zone - 1] - hand, 0) per cell; NaN where hand is NaN or zone < 1 (and where the zone's stage is NaN)"""
    hand = np.asarray(hand, np.float64)
    zone = np.asarray(zone)
    stage = np.asarray(stage, np.float64)
    inside = zone >= 1
    level = np.full(hand.shape, np.nan)
    level[inside] = stage[zone[inside] - 1]
    with np.errstate(invalid='ignore'):
        depth = np.maximum(level - hand, 0.0)           # (np.maximum keeps NaN)
    return depth
