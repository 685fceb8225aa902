"""The host side of DEMProcessor.calc_stream_network: the raw planes of pydem_stream_network (include/pydem_hip.h) compacted
to link ids 1..K, and the table of links.  Plain numpy on planes: nothing here needs a device."""
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
