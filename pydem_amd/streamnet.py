"""The host side of DEMProcessor.calc_stream_network and calc_reach_attributes: the raw planes of pydem_stream_network
(include/pydem_hip.h) compacted to link ids 1..K, the table of links, and the table of per-reach attributes -- the channel
columns from the planes, the catchment columns from what pydem_tree_accum left at the link tails.  Plain numpy on planes:
nothing here needs a device."""
import numpy as np

LINK_DTYPE = np.dtype([('id', np.int32), ('head', np.int64), ('tail', np.int64), ('order', np.int32), ('n_cells', np.int64),
                       ('down', np.int32)])


class StreamNetwork(object):
    """receiver, order, link, basin: int32 planes (basin: None when it was not asked for); links: one row per link (LINK_DTYPE).
    receiver[c]: the flat index of the cell that c's heaviest out-edge leads to, or -1.  order: Strahler, 0 off the streams.
    link, basin: ids 1..K in ascending head-cell order, 0 off the streams / where nothing is reached, -1 where circular drainage
    left the cell unresolved."""

    def __init__(self, receiver, order, link, basin, links):
        self.receiver, self.order, self.link, self.basin, self.links = receiver, order, link, basin, links

    def __repr__(self):
        return "StreamNetwork(%d links, max order %d)" % (self.links.size, int(self.order.max()) if self.order.size else 0)


def compact_labels(raw, labels):
    """raw labels (head cell + 1; 0 and -1 stay) -> ids: the position of the label in the sorted `labels`, + 1"""
    raw = np.asarray(raw)
    out = np.zeros(raw.shape, np.int32)
    pos = raw > 0
    out[pos] = np.searchsorted(labels, raw[pos]) + 1
    out[raw < 0] = -1
    return out


def compact_network(receiver, order, link_raw, basin_raw=None):
    """The planes of pydem_stream_network -> StreamNetwork.  Link ids are 1..K in ascending head-cell order; `down` of a link is
    the id of the link that the receiver of its tail belongs to, 0 if that receiver is off the streams or -1 (no receiver), -1
    if it is an unresolved stream cell."""
    receiver = np.ascontiguousarray(receiver, np.int32)
    order = np.ascontiguousarray(order, np.int32)
    link_raw = np.asarray(link_raw)
    shape = link_raw.shape
    labels = np.unique(link_raw[link_raw > 0])
    K = labels.size
    link = compact_labels(link_raw, labels)
    basin = None if basin_raw is None else compact_labels(basin_raw, labels)
    links = np.zeros(K, LINK_DTYPE)
    links['id'] = np.arange(1, K + 1)
    links['head'] = labels.astype(np.int64) - 1
    lf, rf, of = link.ravel(), receiver.ravel(), order.ravel()
    cells = np.flatnonzero(lf > 0)
    links['n_cells'] = np.bincount(lf[cells], minlength=K + 1)[1:]
    links['order'] = of[links['head']]
    # the tail: the one cell of a link whose receiver is not in the link
    r = rf[cells]
    down = np.where(r >= 0, lf[np.maximum(r, 0)], 0)
    last = down != lf[cells]
    links['tail'][lf[cells[last]] - 1] = cells[last]
    links['down'][lf[cells[last]] - 1] = down[last]
    return StreamNetwork(receiver.reshape(shape), order.reshape(shape), link, basin, links)


REACH_COLUMNS = [('id', np.int32), ('length', np.float64), ('drop', np.float64), ('slope', np.float64), ('straight', np.float64),
                 ('local_cells', np.float64), ('local_area', np.float64), ('total_area', np.float64), ('magnitude', np.float64),
                 ('complete', np.bool_)]
VALUE_COLUMNS = [('v_sum', np.float64), ('v_mean', np.float64), ('v_min', np.float64), ('v_max', np.float64)]
REACH_DTYPE = np.dtype(REACH_COLUMNS)
REACH_VALUES_DTYPE = np.dtype(REACH_COLUMNS + VALUE_COLUMNS)
DEVICE_COLUMNS = ('local_cells', 'local_area', 'total_area', 'magnitude')
DEVICE_VALUE_COLUMNS = ('v_sum', 'v_min', 'v_max')


def magnitude_load(net):
    """the load of the Shreve magnitude: 1 at the heads of the links of order 1 (the sources: a link that starts at a junction
    has order >= 2), 0 elsewhere"""
    load = np.zeros(net.link.shape, np.float64)
    load.ravel()[net.links['head'][net.links['order'] == 1]] = 1.0
    return load


def channel_attributes(net, elev, dX2, dY2):
    """(length, drop, slope, straight) per link, from the planes of `net`, the elevation and the per-row cell sizes dX2 (along
    the columns' index: east-west) and dY2 (north-south).
    length: the sum over the link's cells whose receiver lies in the same link of hypot(dj * dX2[i], di * dY2[i]) for the step
    (di, dj) from the cell (row i) to its receiver -- the spacing of the SOURCE row, as the flow distances use it; a pit step of
    any offset counts with its offset.  drop: elev[head] - elev[tail].  slope: drop / length, NaN where length == 0.
    straight: head (ih, jh) to tail (it, jt) with lo = min(ih, it), hi = max(ih, it):
        hypot((jt - jh) * mean(dX2[lo .. hi]), sum(dY2[lo .. hi - 1]))
    -- the north-south extent is the sum of the heights of the rows stepped out of, the east-west extent uses the mean cell width
    of the rows spanned; under uniform spacing this is hypot((jt - jh) dX, (it - ih) dY)."""
    links = net.links
    K = links.size
    n, m = net.link.shape
    dX2, dY2 = np.asarray(dX2, np.float64), np.asarray(dY2, np.float64)
    lf, rf = net.link.ravel(), net.receiver.ravel().astype(np.int64)
    cells = np.flatnonzero(lf > 0)
    r = rf[cells]
    inside = (r >= 0) & (lf[np.maximum(r, 0)] == lf[cells])
    c, r = cells[inside], r[inside]
    i = c // m
    step = np.hypot((r % m - c % m) * dX2[i], (r // m - i) * dY2[i])
    length = np.bincount(lf[c], weights=step, minlength=K + 1)[1:].astype(np.float64)
    if np.ma.isMaskedArray(elev):
        elev = np.ma.filled(elev.astype(np.float64), np.nan)
    zf = np.asarray(elev, np.float64).ravel()
    head, tail = links['head'], links['tail']
    drop = zf[head] - zf[tail]
    with np.errstate(divide='ignore', invalid='ignore'):
        slope = np.where(length > 0, drop / length, np.nan)
    ih, it = head // m, tail // m
    lo, hi = np.minimum(ih, it), np.maximum(ih, it)
    cx, cy = np.r_[0.0, np.cumsum(dX2)], np.r_[0.0, np.cumsum(dY2)]
    width = (cx[hi + 1] - cx[lo]) / (hi - lo + 1)
    straight = np.hypot((tail % m - head % m) * width, cy[hi] - cy[lo])
    return length, drop, slope, straight


def reach_table(net, elev, dX2, dY2, at_tails):
    """The table of calc_reach_attributes: one row per link of `net`, in the order of net.links.  at_tails: {'local_cells',
    'local_area', 'total_area', 'magnitude'[, 'v_sum', 'v_min', 'v_max']} -> the K values pydem_tree_accum gathered at the link
    tails.  complete = local_area is finite; v_mean = v_sum / local_cells."""
    K = net.links.size
    with_values = any(k in at_tails for k in DEVICE_VALUE_COLUMNS)
    names = DEVICE_COLUMNS + (DEVICE_VALUE_COLUMNS if with_values else ())
    missing = [k for k in names if k not in at_tails]
    if missing:
        raise ValueError("reach_table: no values for %s" % ', '.join(missing))
    out = np.zeros(K, REACH_VALUES_DTYPE if with_values else REACH_DTYPE)
    out['id'] = net.links['id']
    out['length'], out['drop'], out['slope'], out['straight'] = channel_attributes(net, elev, dX2, dY2)
    for k in names:
        v = np.asarray(at_tails[k], np.float64)
        if v.shape != (K,):
            raise ValueError("reach_table: %s holds %r values for %d links" % (k, v.shape, K))
        out[k] = v
    out['complete'] = np.isfinite(out['local_area'])
    if with_values:
        with np.errstate(divide='ignore', invalid='ignore'):
            out['v_mean'] = out['v_sum'] / out['local_cells']
    return out
