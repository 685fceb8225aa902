"""The analyses on a tile's resident flow graph, as the mixin `DEMProcessor` inherits: weighted accumulation, distances down
and up, reverse and forward accumulation, the stream network, receiver-tree accumulation and the reach table.  None has a
counterpart in the reference class.

Every method validates its arguments on the host first (ValueError, no device work), then goes through the one preamble
`_on_flow_graph`: the guard for the drainage alternatives the device path does not have, calc_uca if the tile has no flow
graph yet, the tile handle and the log line.
"""
import logging
import warnings

import numpy as np

from . import _ffi

logger = logging.getLogger(__package__ + '.dem_processing')       # the logger of the class these methods belong to


def _refuse_drain_alternatives(dp):
    if not dp.drain_pits and (dp.drain_flats or dp.drain_pits_spill):
        # (_mk_connectivity_flats / _mk_connectivity_pits_spill, dem_processing.py:1108-1123: alternatives the
        # reference itself labels "not a great option"; only reachable with drain_pits=False)
        raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                  "device path; use drain_pits=True (the reference default) or leave both off")


def _as_plane(value, shape, what, dtype, fill, scalars=False, refuse=None, unreadable=None):
    """`value` as a C-contiguous plane of `shape` and `dtype` (np.float64 or bool); ValueError where it is none.  Masked cells
    become `fill`; a scalar broadcasts with `scalars`; refuse: None, 'nan' or 'nonfinite' values; unreadable: the message for
    a value numpy cannot convert (None: numpy's own error stands)."""
    if np.ma.isMaskedArray(value):
        value = np.ma.filled(value.astype(dtype), fill)
    try:
        a = np.asarray(value) if dtype is bool else np.asarray(value, dtype=dtype)
    except (TypeError, ValueError):
        if unreadable is None:
            raise
        raise ValueError(unreadable)
    if scalars and a.ndim == 0:
        a = np.full(shape, a)
    if a.shape != shape:
        raise ValueError("%s of shape %r for a tile of shape %r" % (what, a.shape, shape))
    if refuse == 'nonfinite' and not np.isfinite(a).all():
        raise ValueError("%s must be finite (%d NaN / inf values)" % (what, int((~np.isfinite(a)).sum())))
    if refuse == 'nan' and np.isnan(a).any():
        raise ValueError("%s must not be NaN (%d NaN values)" % (what, int(np.isnan(a).sum())))
    if dtype is bool:
        a = a.astype(bool)                     # (a mask of any dtype; always a copy of the caller's array)
    return np.ascontiguousarray(a)


def _check_kind_stat(kind, stat):
    if kind not in _ffi.Tile.DIST_KINDS:
        raise ValueError("kind must be one of 'h', 'v', 's' (got %r)" % (kind,))
    if stat not in _ffi.Tile.DIST_STATS:
        raise ValueError("stat must be one of 'ave', 'min', 'max' (got %r)" % (stat,))


class FlowAnalyses(object):
    """The flow-graph methods of DEMProcessor, their result and stats attributes and their helpers."""

    def _on_flow_graph(self, starting):
        """The opening of every analysis, after its arguments are checked: the tile, holding the flow graph of calc_uca."""
        _refuse_drain_alternatives(self)
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the analysis runs on (kept, with uca: nothing is thrown away)
        tile = self._ensure_tile()
        logger.info("Starting " + starting)
        return tile

    def _weights_array(self, weights):
        """float64 weights of the tile's shape (scalars broadcast, masked cells 0); ValueError before any device work."""
        return _as_plane(weights, tuple(self.shape), 'weights', np.float64, 0.0, scalars=True, refuse='nonfinite')

    def _plane_array(self, values, what, neutral):
        """float64 plane of the tile's shape (scalars broadcast, masked cells `neutral`); ValueError before any device work.
        NaN is refused here; what else the values must satisfy is the caller's to check."""
        return _as_plane(values, tuple(self.shape), what, np.float64, neutral, scalars=True, refuse='nan',
                         unreadable="%s must be a number or an array of numbers" % what)

    def _mask_array(self, mask, what):
        """boolean mask of the tile's shape (masked cells False); ValueError before any device work."""
        return _as_plane(mask, tuple(self.shape), what, bool, False)

    def _stream_set(self, target, uca_threshold):
        """(mask or None, threshold or None) after the checks that need no device; ValueError otherwise."""
        if (target is None) == (uca_threshold is None):
            raise ValueError("give exactly one of target (a mask) and uca_threshold")
        if target is not None:
            return self._mask_array(target, 'target'), None
        try:
            thr = float(uca_threshold)
        except (TypeError, ValueError):
            raise ValueError("uca_threshold must be a number (got %r)" % (uca_threshold,))
        if not np.isfinite(thr) or thr < 0:
            raise ValueError("uca_threshold must be finite and >= 0 (got %r)" % (uca_threshold,))
        return None, thr

    def _outlets_mask(self, outlets):
        """`outlets` -- a boolean mask of the tile's shape, or a sequence of (row, col) pairs -- as a boolean mask; ValueError
        before any device work."""
        shape = tuple(self.shape)
        arr = outlets if np.ma.isMaskedArray(outlets) else np.asarray(outlets)
        pairs = arr.ndim == 2 and arr.shape[1] == 2 and arr.dtype.kind in 'iu'
        if arr.shape == shape and (arr.dtype.kind == 'b' or not pairs):
            return self._mask_array(arr, 'outlets')
        if pairs or arr.size == 0:
            arr = arr.reshape(-1, 2).astype(np.int64)
            rows, cols = arr[:, 0], arr[:, 1]
            bad = (rows < 0) | (rows >= shape[0]) | (cols < 0) | (cols >= shape[1])
            if bad.any():
                raise ValueError("outlet %r is outside the tile of shape %r" % (tuple(int(v) for v in arr[np.argmax(bad)]), shape))
            mask = np.zeros(shape, bool)
            mask[rows, cols] = True
            return mask
        raise ValueError("outlets must be a mask of shape %r or a sequence of (row, col) pairs of integers (got shape %r, dtype %s)"
                         % (shape, arr.shape, arr.dtype))

    def _cell_area_plane(self):
        return np.ascontiguousarray(np.broadcast_to((self.dX2 * self.dY2)[:, None], tuple(self.shape)))

    # ------------------------------------------------------------------ weighted accumulation
    def calc_weighted_uca(self, weights, scale_by_cell_area=True):
        """Weighted flow accumulation along the D-infinity flow graph of calc_uca: the reference's sweep (_calc_uca_chunk
        :864-987, cyutils.pyx:119-187) started from w * dX2 * dY2 (scale_by_cell_area) or w per cell instead of the cell area,
        like TauDEM's AreaDinf with a weight grid -- pit drains, the on-edge skip and the circular-drainage re-seed loop
        included, NaN on flats.  `weights`: a scalar or an array of the tile's shape, any finite values (zero and negative
        ones too); masked cells count as 0.  With weights = 1 the result is `uca` bit for bit.  Returns the float64 array."""
        self.run_weighted_uca(weights, scale_by_cell_area)
        return self.uca_weighted

    def run_weighted_uca(self, weights, scale_by_cell_area=True):
        """calc_weighted_uca without bringing the result back to the host (the `uca_weighted` attribute).  Leaves uca,
        mag, flats, the edge masks and twi_min_area alone.  The flow graph is the one calc_uca would build with the current
        options: the tile's own after calc_uca, built for the call (and not kept) otherwise."""
        w = self._weights_array(weights)
        _refuse_drain_alternatives(self)
        if not self._has('direction'):
            self.run_slopes_directions()
        self._ensure_tile()
        self._push('elev', 'mag', 'direction', 'flats')
        self._tile.upload(_ffi.WEIGHT, w)
        logger.info("Starting weighted uca calculation")
        self._tile.uca_weighted(self._options(), scale_by_cell_area)
        # (a graph the call had to build itself is not kept: section, proportion, mag, flats, edge_todo are as they were)
        self._produced('uca_weighted')

    # ------------------------------------------------------------------ distances
    dist_down = None      # last calc_dist_down (no counterpart in the reference)
    hand = None           # last calc_hand
    dist_down_stats = None    # {'ms', 'levels', 'n_unresolved', 'kind', 'stat'} of the last calc_dist_down / calc_hand

    def calc_dist_down(self, target=None, uca_threshold=None, kind='h', stat='ave'):
        """Distance along the D-infinity flow paths of calc_uca down to the nearest target cells (TauDEM's DinfDistDown; no
        reference method).  Targets: `target`, a boolean mask of the tile's shape (masked cells are no targets), or
        `uca_threshold`: the cells with uca >= uca_threshold (the streams) -- exactly one of the two.  kind: 'h' horizontal
        distance, 'v' drop in elevation (signed), 's' distance along the surface; stat: 'ave' (flow-weighted mean over the
        out-edges), 'min' or 'max'.  NaN where some flow path from the cell does not end in a target inside the tile (it
        leaves the tile, or ends in an undrained pit or flat) and on or upstream of a drainage cycle.  Runs on the flow
        graph of calc_uca (computed first if the tile has none).  Returns the float64 array, kept as `dist_down`."""
        res = self._dist_down(target, uca_threshold, kind, stat)
        self.dist_down = res
        return res

    def calc_hand(self, uca_threshold=None, target=None):
        """Height above the nearest drainage: calc_dist_down with kind='v', stat='ave'.  Kept as `hand`."""
        res = self._dist_down(target, uca_threshold, 'v', 'ave')
        self.hand = res
        return res

    def _dist_down(self, target, uca_threshold, kind, stat):
        _check_kind_stat(kind, stat)
        mask, thr = self._stream_set(target, uca_threshold)
        tile = self._on_flow_graph("downslope distance calculation")
        out, ms, levels, left = tile.dist_down(kind, stat, mask, thr)
        self.dist_down_stats = dict(ms=ms, levels=levels, n_unresolved=left, kind=kind, stat=stat)
        if left:
            warnings.warn("%d cells lie on or upstream of a circular drainage pattern: their downslope distance is NaN" % left)
        return out

    dist_up = None        # last calc_dist_up (no counterpart in the reference)
    dist_up_stats = None      # {'ms', 'levels', 'n_unresolved', 'kind', 'stat', 'edge_nan'} of the last calc_dist_up

    def calc_dist_up(self, kind='h', stat='max', edge_nan=True):
        """Distance along the D-infinity flow paths of calc_uca from the divides down to each cell (TauDEM's DinfDistUp; no
        reference method); with stat='max' the longest flow path into the cell.  kind: 'h' horizontal distance, 'v' drop in
        elevation (signed), 's' distance along the surface; stat: 'ave' (flow-weighted mean over the in-edges), 'min' or
        'max'.  0 where nothing flows into the cell, NaN where the elevation is NaN and on or downstream of a drainage cycle.
        edge_nan (TauDEM's edge contamination): the tile's border cells and the neighbours of no-data cells are NaN, and so
        is everything downstream of them -- a value is finite only where no flow path into the cell can start outside the
        tile's data; edge_nan=False gives the values of the paths inside the tile (a lower bound for 'max').  Runs on the flow
        graph of calc_uca (computed first if the tile has none).  Returns the float64 array, kept as `dist_up`."""
        _check_kind_stat(kind, stat)
        tile = self._on_flow_graph("upslope distance calculation")
        edge_nan = bool(edge_nan)
        out, ms, levels, left = tile.dist_up(kind, stat, edge_nan)
        self.dist_up_stats = dict(ms=ms, levels=levels, n_unresolved=left, kind=kind, stat=stat, edge_nan=edge_nan)
        if left:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their upslope distance is NaN" % left)
        self.dist_up = out
        return out

    # ------------------------------------------------------------------ reverse accumulation
    up_dependence = None          # last calc_up_dependence / calc_watershed (no counterpart in the reference)
    up_dependence_stats = None    # {'ms', 'levels', 'n_unresolved'} of that call
    watershed = None              # last calc_watershed
    rev_accum = None              # last calc_rev_accum: the weighted sum downslope ...
    rev_accum_max = None          # ... and the maximum downslope
    rev_accum_stats = None        # {'sum': {'ms', 'levels', 'n_unresolved'}, 'max': {...}} of the two calls behind it

    def _rev_accum(self, what, op, seed=None, absorb=None):
        """One pydem_rev_accum call on the flow graph of calc_uca (computed first if the tile has none): (array, stats)."""
        tile = self._on_flow_graph("%s calculation" % what)
        out, ms, levels, left = tile.rev_accum(op, seed, absorb, 1.0)
        if left:
            warnings.warn("%d cells lie on or upstream of a circular drainage pattern: their %s is NaN" % (left, what))
        return out, dict(ms=ms, levels=levels, n_unresolved=left)

    def calc_up_dependence(self, target):
        """Upslope dependence on a target set (TauDEM's DinfUpDependence; no reference method): per cell, the fraction of its
        flow that reaches the targets along the D-infinity flow paths of calc_uca; 1 on the targets, and > 0 exactly on their
        D-infinity watershed.  `target`: a boolean mask of the tile's shape (masked cells are no targets).  Not normalised:
        the share of a cell's flow that leaves the tile, or ends in an undrained pit or flat, reaches nothing.  NaN where the
        elevation is NaN and on or upstream of a drainage cycle.  Runs on the flow graph of calc_uca (computed first if the tile
        has none).  Returns the float64 array, kept as `up_dependence`; `up_dependence_stats` holds the call's device time, levels
        and unresolved cells."""
        mask = self._mask_array(target, 'target')
        out, st = self._rev_accum('upslope dependence', 'sum', None, mask)
        self.up_dependence, self.up_dependence_stats = out, st
        return out

    def calc_watershed(self, outlets, min_fraction=0.0):
        """The D-infinity watershed of `outlets`: the cells of which more than `min_fraction` (in [0, 1)) of the flow reaches
        an outlet -- calc_up_dependence and a comparison (NaN is outside, the outlets themselves inside).  `outlets`: a
        boolean mask of the tile's shape, or a sequence of (row, col) pairs.  Returns the boolean mask, kept as `watershed`;
        `up_dependence` is set too."""
        try:
            frac = float(min_fraction)
        except (TypeError, ValueError):
            raise ValueError("min_fraction must be a number in [0, 1) (got %r)" % (min_fraction,))
        if not (0.0 <= frac < 1.0):
            raise ValueError("min_fraction must be in [0, 1) (got %r)" % (min_fraction,))
        mask = self._outlets_mask(outlets)
        dep = self.calc_up_dependence(mask)
        with np.errstate(invalid='ignore'):
            self.watershed = dep > frac
        return self.watershed

    def calc_rev_accum(self, weights):
        """Reverse accumulation of a per-cell load (TauDEM's DinfRevAccum; no reference method): (racc, dmax), the
        flow-weighted sum and the maximum of `weights` over the cell itself and everything downslope of it along the
        D-infinity flow paths of calc_uca.  `weights`: a scalar or an array of the tile's shape, any finite values; masked
        cells count as 0.  The sum is not normalised: flow that leaves the tile carries nothing back.  NaN where the
        elevation is NaN and on or upstream of a drainage cycle.  Runs on the flow graph of calc_uca (computed first if the tile
        has none).  Kept as `rev_accum` and `rev_accum_max`; `rev_accum_stats` holds the stats of both calls."""
        w = self._weights_array(weights)
        racc, st_sum = self._rev_accum('reverse accumulation', 'sum', w, None)
        dmax, st_max = self._rev_accum('maximum downslope load', 'max', w, None)
        self.rev_accum, self.rev_accum_max = racc, dmax
        self.rev_accum_stats = dict(sum=st_sum, max=st_max)
        return racc, dmax

    # ------------------------------------------------------------------ forward accumulation
    decay_accum = None            # last calc_decay_accum (no counterpart in the reference)
    decay_accum_stats = None      # {'ms', 'levels', 'n_unresolved', 'edge_nan'} of that call
    trans_lim_accum = None        # last calc_trans_lim_accum: the transport ...
    trans_lim_deposition = None   # ... and the deposition
    trans_lim_stats = None        # {'ms', 'levels', 'n_unresolved', 'edge_nan'} of that call

    def _fwd_accum(self, what, load, mult, cap, edge_nan, inflow):
        """One pydem_fwd_accum call on the flow graph of calc_uca (computed first if the tile has none): (array, inflow or
        None, stats)."""
        tile = self._on_flow_graph("%s calculation" % what)
        edge_nan = bool(edge_nan)
        out, flow, ms, levels, left = tile.fwd_accum(load, mult, cap, edge_nan, inflow)
        if left:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their %s is NaN" % (left, what))
        return out, flow, dict(ms=ms, levels=levels, n_unresolved=left, edge_nan=edge_nan)

    def calc_decay_accum(self, weights, decay=None, edge_nan=True):
        """Accumulation of a per-cell load that decays on its way down (TauDEM's DinfDecayAccum; no reference method): every
        cell holds its own `weights` plus, over the D-infinity in-edges of calc_uca, the flow-weighted share of decay x the
        value of the cells that flow into it.  `weights`: a scalar or an array of the tile's shape, any finite values; masked
        cells count as 0.  `decay`: the share of a cell's value that leaves it, a scalar or an array in [0, 1] (masked cells
        1), or None: the plain weighted accumulation over the graph's in-edges.  The values are the tile's own: nothing enters
        through the border.  NaN where the elevation is NaN and on or downstream of a drainage cycle.  edge_nan (TauDEM's edge
        contamination, as in calc_dist_up): the tile's border cells and the neighbours of no-data cells are NaN, and so is
        everything downstream of them -- a value is finite only where it is complete, because no flow path into the cell can
        start outside the tile's data.  Runs on the flow graph of calc_uca (computed first if the tile has none).  Returns the
        float64 array, kept as `decay_accum`; `decay_accum_stats` holds the call's device time, levels and unresolved cells."""
        w = self._weights_array(weights)
        k = None
        if decay is not None:
            k = self._plane_array(decay, 'decay', 1.0)
            if not ((k >= 0.0) & (k <= 1.0)).all():
                raise ValueError("decay must be in [0, 1] (%d values outside)" % int((~((k >= 0.0) & (k <= 1.0))).sum()))
        out, _, st = self._fwd_accum('decaying accumulation', w, k, None, edge_nan, False)
        self.decay_accum, self.decay_accum_stats = out, st
        return out

    def calc_trans_lim_accum(self, supply, capacity, edge_nan=True):
        """Transport-limited accumulation (TauDEM's DinfTransLimAccum; no reference method): (transport, deposition).  Every cell
        receives its own `supply` plus the flow-weighted transport of the cells that flow into it along the D-infinity in-edges
        of calc_uca, passes on min(that, `capacity`) -- the transport -- and keeps the rest -- the deposition, (supply + inflow)
        - transport: exactly 0 wherever the capacity does not bind, never negative.  `supply`: a scalar or an array of the
        tile's shape, finite and >= 0 (masked cells 0); `capacity`: the same, >= 0, +inf allowed (masked cells +inf).  The
        values are the tile's own; NaN, edge_nan and the flow graph as for calc_decay_accum.  Kept as `trans_lim_accum` and
        `trans_lim_deposition`; `trans_lim_stats` holds the call's device time (sweep and inflow pass), levels and unresolved cells."""
        s = self._plane_array(supply, 'supply', 0.0)
        if not (np.isfinite(s).all() and (s >= 0.0).all()):
            raise ValueError("supply must be finite and >= 0 (%d values are not)" % int((~(np.isfinite(s) & (s >= 0.0))).sum()))
        cap = self._plane_array(capacity, 'capacity', np.inf)
        if not (cap >= 0.0).all():
            raise ValueError("capacity must be >= 0 (%d negative values)" % int((cap < 0.0).sum()))
        transport, inflow, st = self._fwd_accum('transport-limited accumulation', s, None, cap, edge_nan, True)
        with np.errstate(invalid='ignore'):
            deposition = (s + inflow) - transport
        self.trans_lim_accum, self.trans_lim_deposition, self.trans_lim_stats = transport, deposition, st
        return transport, deposition

    # ------------------------------------------------------------------ stream network
    flow_receiver = None          # last calc_flow_receiver (no counterpart in the reference)
    stream_network = None         # last calc_stream_network: a streamnet.StreamNetwork
    stream_network_stats = None   # {'ms', 'levels', 'n_unresolved', 'n_links', 'max_order'} of that call

    def _stream_network(self, mask, thr, **planes):
        """One pydem_stream_network call on the flow graph of calc_uca (computed first if the tile has none)."""
        return self._on_flow_graph("stream network calculation").stream_network(mask, thr, **planes)

    def calc_flow_receiver(self):
        """The receiver of every cell: the flat index (row * n_cols + col) of the cell its heaviest D-infinity out-edge leads to
        -- the first of greatest weight in ascending destination order, a regular edge before a pit edge to the same cell --,
        -1 where the cell has no out-edge or no data.  The receivers pick the one tree the flow graph of calc_uca (computed
        first if the tile has none) contains.  Returns the int32 array, kept as `flow_receiver`."""
        planes, _, _, _ = self._stream_network(None, None, receiver=True, order=False, link=False, basin=False)
        self.flow_receiver = planes['receiver']
        return self.flow_receiver

    def calc_stream_network(self, uca_threshold=None, streams=None, basins=True):
        """The stream network on the flow graph of calc_uca (TauDEM's StreamNet / GridNet, there on D8; no reference method).
        The streams: the cells with uca >= `uca_threshold`, or `streams`, a boolean mask of the tile's shape (masked cells are
        no streams) -- exactly one of the two.  Stream cells are joined along the receivers of calc_flow_receiver: `order` is
        the Strahler order (0 off the streams), `link` the id of the reach between two junctions (a cell with other than one
        stream inflow starts a link), `basin` the id of the link that a cell's receivers lead to (0: none; None with
        basins=False), `links` a structured array with one row per link: id (1..K in ascending head-cell order), head, tail
        (flat cells), order, n_cells and down, the id of the link below (0: none).  -1 in order, link and basin marks cells
        that circular drainage left unresolved.  Returns the streamnet.StreamNetwork, kept as `stream_network`;
        `stream_network_stats` holds the device times (receiver pass, forward sweep, reverse sweep), the levels and the
        unresolved cells of the two sweeps, the number of links and the greatest order."""
        from . import streamnet
        mask, thr = self._stream_set(streams, uca_threshold)
        planes, ms, levels, left = self._stream_network(mask, thr, receiver=True, order=True, link=True, basin=bool(basins))
        net = streamnet.compact_network(planes['receiver'], planes['order'], planes['link'], planes['basin'])
        self.flow_receiver, self.stream_network = net.receiver, net
        self.stream_network_stats = dict(ms=ms, levels=levels, n_unresolved=left, n_links=int(net.links.size),
                                         max_order=int(net.order.max()) if net.order.size else 0)
        if any(left):
            warnings.warn("%d stream cells lie on or downstream of a circular drainage pattern (order and link are -1) and %d "
                          "cells lead into it (basin is -1)" % left)
        return net

    # ------------------------------------------------------------------ receiver tree
    tree_accum = None             # last calc_tree_accum (no counterpart in the reference)
    tree_accum_stats = None       # {'ms', 'levels', 'n_unresolved', 'edge_nan', 'cut'} of that call
    reach_attributes = None       # last calc_reach_attributes: one row per link of `stream_network`
    reach_attributes_stats = None     # {'ms', 'sweeps': {column: {'ms', 'levels', 'n_unresolved'}}, 'edge_nan', 'n_links'}

    def _tree_accum(self, load, op, mask, thr, edge_nan, at=None, download=True):
        """One pydem_tree_accum call on the flow graph of calc_uca (computed first if the tile has none): (array or None, values
        at `at` or None, stats)."""
        tile = self._on_flow_graph("receiver-tree accumulation")
        edge_nan = bool(edge_nan)
        out, vals, ms, levels, left = tile.tree_accum(load, op, mask, thr, edge_nan, at, download)
        return out, vals, dict(ms=ms, levels=levels, n_unresolved=left, edge_nan=edge_nan, cut=mask is not None or thr is not None)

    def calc_tree_accum(self, weights=None, op='sum', streams=None, uca_threshold=None, edge_nan=True):
        """Accumulation along the receiver tree (the single-flow-direction, D8-style accumulation on the steepest D-infinity
        receiver of calc_flow_receiver; no reference method): every cell holds the `op` ('sum', 'max' or 'min') of its own
        `weights` and the values of the cells whose receiver it is.  `weights`: a scalar or an array of the tile's shape, any
        finite values (masked cells 0), or None: the cell area dX2 * dY2, which makes the sum the D8-style contributing area.
        With a stream set -- `streams`, a boolean mask of the tile's shape, or `uca_threshold`, not both -- the accumulation is
        cut at the link boundaries of calc_stream_network: a stream cell passes its value on only to the cell that continues its
        link, so the value at a link's tail is the reduction over that link's own sub-basin.  NaN where the elevation is NaN
        and on or downstream of a drainage cycle.  edge_nan (as in calc_dist_up): the tile's border cells and the neighbours of
        no-data cells are NaN, and so is what their values reach along the tree -- a cut stops that too, so a finite value
        under a cut says the link's own catchment lies inside the tile's data.  Runs on the flow graph of calc_uca (computed
        first if the tile has none).  Returns the float64 array, kept as `tree_accum`; `tree_accum_stats` holds the call's
        device time, levels, unresolved cells, edge_nan and cut."""
        if op not in _ffi.Tile.TREE_OPS:
            raise ValueError("op must be one of 'sum', 'max', 'min' (got %r)" % (op,))
        if streams is not None and uca_threshold is not None:
            raise ValueError("give at most one of streams (a mask) and uca_threshold")
        mask = thr = None
        if streams is not None or uca_threshold is not None:
            mask, thr = self._stream_set(streams, uca_threshold)
        w = self._cell_area_plane() if weights is None else self._weights_array(weights)
        out, _, st = self._tree_accum(w, op, mask, thr, edge_nan)
        if st['n_unresolved']:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their tree accumulation is NaN" % st['n_unresolved'])
        self.tree_accum, self.tree_accum_stats = out, st
        return out

    def calc_reach_attributes(self, uca_threshold=None, streams=None, values=None, edge_nan=True):
        """The attribute table of the stream network's reaches (TauDEM's StreamNet table; no reference method).  Runs
        calc_stream_network(basins=False) for the stream set -- `uca_threshold` or `streams`, exactly one -- and then one
        receiver-tree accumulation (calc_tree_accum's) per catchment column, each read at the link tails only.  Returns a
        structured array with one row per link, in the order of `stream_network.links`:
            id; length, the channel length along the receivers (streamnet.channel_attributes states the formulas); drop =
            elev[head] - elev[tail]; slope = drop / length (NaN for a one-cell link); straight, the head-to-tail distance;
            local_cells / local_area, the cells / area of the link's own sub-basin (cut at the link boundaries); total_area, the
            area of everything whose receivers lead to the link's tail; magnitude, the Shreve magnitude (the sources above the
            tail); complete = local_area is finite; with `values` (an array of the tile's shape, masked cells NaN, NaN allowed)
            also v_sum, v_mean = v_sum / local_cells, v_min and v_max of it over the link's own sub-basin.
        The catchment columns are the tile's own: with edge_nan a column is NaN where the cells it covers may continue beyond
        the tile's data (for the cut columns: only this link's sub-basin), and on or downstream of circular drainage.  Kept as
        `reach_attributes`; `reach_attributes_stats` holds the device time of all sweeps and the stats of each."""
        from . import streamnet
        mask, thr = self._stream_set(streams, uca_threshold)
        vals = None
        if values is not None:
            vals = _as_plane(values, tuple(self.shape), 'values', np.float64, np.nan, unreadable="values must be an array of numbers")
        net = self.calc_stream_network(uca_threshold=thr, streams=mask, basins=False)
        tails = net.links['tail']
        area = self._cell_area_plane()
        ones = np.ones(tuple(self.shape), np.float64)
        sweeps = [('local_cells', ones, 'sum', True), ('local_area', area, 'sum', True), ('total_area', area, 'sum', False),
                  ('magnitude', streamnet.magnitude_load(net), 'sum', False)]
        if vals is not None:
            sweeps += [('v_sum', vals, 'sum', True), ('v_min', vals, 'min', True), ('v_max', vals, 'max', True)]
        at_tails, stats = {}, {}
        for name, load, op, cut in sweeps:
            _, at_tails[name], st = self._tree_accum(load, op, mask if cut else None, thr if cut else None, edge_nan, tails, False)
            stats[name] = dict(ms=st['ms'], levels=st['levels'], n_unresolved=st['n_unresolved'])
        table = streamnet.reach_table(net, self.elev, self.dX2, self.dY2, at_tails)
        self.reach_attributes = table
        self.reach_attributes_stats = dict(ms=sum(st['ms'] for st in stats.values()), sweeps=stats, edge_nan=bool(edge_nan),
                                           n_links=int(table.size))
        return table

    # ------------------------------------------------------------------ HAND hydraulics
    hand_hydraulics = None        # last calc_hand_hydraulics: a hydraulics.HandHydraulics (no counterpart in the reference)
    hand_hydraulics_stats = None  # {'ms': {part: device ms}, 'n_links', 'n_stages', 'n_unresolved'} of that call
    inundation = None             # last calc_inundation

    def calc_hand_hydraulics(self, stages, uca_threshold=None, streams=None, manning_n=0.05, edge_nan=True):
        """The HAND hydraulic property table and the synthetic rating curve of every reach (the step that follows HAND in the CFIM
        / NWM HAND workflows; no reference method).  `stages`: 1 .. 1024 water stages above the drainage, finite and strictly
        ascending.  The streams: `uca_threshold` or `streams` (a boolean mask), exactly one, as for calc_stream_network.  Runs
        calc_reach_attributes for each reach's length and slope, calc_stream_network for the catchment (basin) of each reach, the
        HAND sweep of calc_hand, left on the device, and one reduction of that plane over (basin, stage) (pydem_hand_table,
        include/pydem_hip.h: fixed-point sums, one result whatever the schedule).  Returns a hydraulics.HandHydraulics with one
        row per link of `stream_network`: per stage the flooded cells, area, volume and wetted bed area of the link's catchment,
        the reach-averaged top width, cross-section, wetted perimeter and hydraulic radius, and the discharge by Manning's
        equation with `manning_n` (NaN for a link without a positive slope or length); cells_nan / cells_above count the
        catchment's cells whose HAND is NaN / above the top stage.  Per tile: a catchment cut by the tile's border is what the
        tile holds of it (`reach_attributes['complete']` tells).  Kept as `hand_hydraulics`; `hand_hydraulics_stats` holds the
        device milliseconds per part."""
        from . import hydraulics
        st = hydraulics.check_stages(stages)
        try:
            n_man = float(manning_n)
        except (TypeError, ValueError):
            raise ValueError("manning_n must be a number > 0 (got %r)" % (manning_n,))
        if not (n_man > 0 and np.isfinite(n_man)):
            raise ValueError("manning_n must be finite and > 0 (got %r)" % (manning_n,))
        mask, thr = self._stream_set(streams, uca_threshold)
        reaches = self.calc_reach_attributes(uca_threshold=thr, streams=mask, edge_nan=edge_nan)
        net = self.calc_stream_network(uca_threshold=thr, streams=mask, basins=True)
        K = int(net.links.size)
        tile = self._on_flow_graph("HAND hydraulic table calculation")
        _, dd_ms, _, left = tile.dist_down('v', 'ave', mask, thr, download=False)
        ints, skipped, quanta, ms = tile.hand_table(net.basin, st, K, hand=None)
        table = hydraulics.hydraulic_table(ints, quanta, st, reaches['length'], reaches['slope'], n_man)
        res = hydraulics.HandHydraulics(st, net.links['id'], table, skipped[:, 0], skipped[:, 1], reaches['length'], reaches['slope'],
                                        ints=ints, skipped=skipped, quanta=quanta, zone=net.basin, manning_n=n_man)
        res.stream_set = (mask, thr)
        self.hand_hydraulics = res
        self.hand_hydraulics_stats = dict(
            ms=dict(reach_attributes=self.reach_attributes_stats['ms'], stream_network=float(sum(self.stream_network_stats['ms'])),
                    dist_down=dd_ms, hand_table=ms['total'], hand_table_maxima=ms['maxima'], hand_table_sums=ms['sums']),
            n_links=K, n_stages=int(st.size), n_unresolved=left)
        if left:
            warnings.warn("%d cells lie on or upstream of a circular drainage pattern: their HAND is NaN" % left)
        return res

    def calc_inundation(self, stage=None, discharge=None):
        """The inundation depth map of `hand_hydraulics` (calc_hand_hydraulics first) for a water `stage` above the drainage or a
        `discharge` -- exactly one, a scalar for every link or one value per link.  A discharge becomes the stage of each link by
        linear interpolation over the finite points of its rating curve: below the first point the first stage, above the last
        NaN (no extrapolation), NaN with a warning where the rating is not non-decreasing.  The depth of a cell is
        max(stage of its basin's link - HAND, 0); NaN where HAND is NaN and where the cell belongs to no basin.  Host numpy on
        the HAND plane of calc_hand and the basin plane.  Returns the float64 array, kept as `inundation`."""
        from . import hydraulics
        if (stage is None) == (discharge is None):
            raise ValueError("give exactly one of stage and discharge")
        hh = self.hand_hydraulics
        if hh is None:
            raise ValueError("calc_inundation needs the table of calc_hand_hydraulics: call it first")
        K = int(hh.link_ids.size)
        what = 'stage' if stage is not None else 'discharge'
        try:
            v = np.asarray(stage if stage is not None else discharge, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number or an array of numbers" % what)
        if v.ndim == 0:
            v = np.full(K, float(v))
        if v.shape != (K,):
            raise ValueError("%s of shape %r for %d links (a scalar, or one value per link)" % (what, v.shape, K))
        level = v if stage is not None else hydraulics.stage_for_discharge(hh.stages, hh.discharge, v)
        if hh.zone is None:
            raise ValueError("calc_inundation: hand_hydraulics holds no basin plane (a table made by hand)")
        if hh.hand is None:
            mask, thr = hh.stream_set
            hh.hand = self.calc_hand(uca_threshold=thr, target=mask)
        self.inundation = hydraulics.inundation_depth(hh.hand, hh.zone, level)
        return self.inundation
