"""CPU tier: what each designed field of tests/flow_fields.py is on the oracle's graph, so that tests/test_gpu_flow_fields.py
cannot go vacuous: the chains and their depth under the three references (dist_down_ref, dist_up_ref, rev_accum_ref), the
single section and the two unequal out-edges of the fans, where the pits drain, and the closed forms the device is held to.
The fields made for the UCA sweep (tests/test_gpu_uca_fields.py) follow: uca along the chains, the partly tainted roofs, the
chains and strips longer than the capped grids."""
import functools

import numpy as np
import pytest

import flow_fields as F
from test_dist_down_ref import dist_down_ref, edge_cost
from test_dist_up_ref import dist_up_ref
from test_rev_accum_ref import rev_accum_ref

SNAKES = ('row_snake', 'tile_snake', 'tall', 'wide')
DEPTH = {'row_snake': 3150, 'tile_snake': 2240, 'tall': 4100, 'wide': 700}


@functools.lru_cache(maxsize=None)
def oracle(name, *args):
    return F.oracle(getattr(F, name)(*args))


def chain_index(f):
    """(cells to the chain's end, the cell itself included; horizontal length of the path from the chain's head) per cell"""
    sp = f.spacing
    to_end = np.zeros(f.elev.shape)
    from_head = np.zeros(f.elev.shape)
    for p in f.facts['paths']:
        step = np.abs(np.diff(p, axis=0))
        length = np.hypot(step[:, 1] * sp['dX'], step[:, 0] * sp['dY'])
        to_end[p[:, 0], p[:, 1]] = len(p) - np.arange(len(p))
        from_head[p[:, 0], p[:, 1]] = np.r_[0.0, np.cumsum(length)]
    return to_end, from_head


@pytest.mark.parametrize('name', SNAKES)
def test_snakes_are_chains_of_the_stated_depth(name):
    f = getattr(F, name)()
    o = oracle(name)
    od = F.out_degree(o)
    NN = f.elev.size
    indptr, indices, data = o.A
    for p in f.facts['paths']:
        assert (np.abs(np.diff(p, axis=0)).sum(axis=1) == 1).all()
        cells = p[:, 0] * f.elev.shape[1] + p[:, 1]
        assert (od.ravel()[cells[:-1]] == 1).all() and od.ravel()[cells[-1]] == 0
        assert np.array_equal(indices[indptr[cells[:-1]]], cells[1:]) and (data == 1.0).all()
    assert sum(len(p) for p in f.facts['paths']) == NN and f.target.sum() == len(f.facts['paths'])
    assert f.facts['depth'] == len(f.facts['path']) == DEPTH[name]
    for what, (_, final, depth) in (('dist_down', dist_down_ref(o, f.target, 'h', 'ave')), ('dist_up', dist_up_ref(o, 'h', 'max', False)),
                                    ('rev_accum', rev_accum_ref(o, 0, seed=1.0))):
        assert final.all() and depth == DEPTH[name], (what, depth)


def test_snake_crossings_and_the_1024_cell_run():
    assert F.row_snake().facts['crossings'] == 70 + 2                    # one per row, and two from row to row
    assert F.tall().facts['crossings'] == 128 and F.wide().facts['crossings'] == 21
    f = F.tile_snake()
    assert f.elev.shape == (40, 70) and [len(p) for p in f.facts['paths']] == [32 * 70, 8 * 70]
    assert f.facts['crossings'] == 2 and f.facts['longest_run'] == 1024 == F.longest_run_in_one_block(f.facts['path'])
    # the ragged blocks: 32 x 6, 8 x 32 and 8 x 6
    assert [F.longest_run_in_one_block(p) for p in f.facts['paths']] == [1024, 256]
    assert F.crossings(f.facts['paths'][1]) == 2 and len(f.facts['paths'][1]) == 256 + 256 + 48
    with pytest.raises(AssertionError, match='ends at the bottom'):
        F.tile_snake.__wrapped__(40, 69)


@pytest.mark.parametrize('name', SNAKES)
def test_closed_forms_on_the_snakes(name):
    f = getattr(F, name)()
    o = oracle(name)
    to_end, from_head = chain_index(f)
    count, final, _ = rev_accum_ref(o, 0, seed=1.0)
    assert final.all() and np.array_equal(count, to_end)
    up, _, _ = dist_up_ref(o, 'h', 'max', False)
    assert np.array_equal(up, from_head)
    dep, _, _ = rev_accum_ref(o, 0, absorb=f.target)
    assert (dep == 1.0).all()
    # (the prefix sums are sums of 2s and 3s: exact, whatever the order)
    cells = f.facts['path'][:, 0] * f.elev.shape[1] + f.facts['path'][:, 1]
    assert from_head.max() == edge_cost(o, cells[:-1], cells[1:], 'h').sum()


@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('k', range(8))
def test_fans_have_one_section_and_two_unequal_out_edges(k, mirror):
    f = F.fan(k, mirror)
    o = oracle('fan', k, mirror)
    assert f.elev.shape == (70, 45)
    want = (3 - k) % 8 if mirror else k
    assert np.array_equal(np.unique(o.section), [want]) and f.facts['section'] == want
    od = F.out_degree(o)
    assert (od == 2).mean() >= 0.90 and np.array_equal(f.target, od < 2)
    assert np.abs(o.A[2] - 0.5).min() > 0.05
    d, final, _ = dist_down_ref(o, f.target, 'h', 'ave')
    assert final.all() and np.isfinite(d).all()
    if mirror:
        assert np.array_equal(f.elev[:, ::-1], F.fan(k).elev) and np.array_equal(f.target[:, ::-1], F.fan(k).target)


@pytest.mark.parametrize('row_varying', [False, True])
def test_far_pit_drains_two_blocks_away(row_varying):
    f = F.far_pit(row_varying)
    o = oracle('far_pit', row_varying)
    n, m = f.elev.shape
    assert (n, m) == (96, 112)
    (pit, dst), = F.pit_edges_kept(o)
    assert divmod(pit, m) == f.facts['pit'] and o.n_warn == 0
    assert len(dst) >= 50
    pb = np.array([pit // m // F.T, pit % m // F.T])
    db = np.c_[dst // m // F.T, dst % m // F.T]
    assert (np.abs(db - pb).max(axis=1) >= 2).all()
    assert len(set(map(tuple, db.tolist()))) >= 3
    if row_varying:
        rows = dst // m
        assert rows.max() - pit // m >= 50 and np.unique(o.dY2[rows]).size >= 40
    # the target of the downslope calls leaves the basin finite
    d, final, _ = dist_down_ref(o, f.target, 'h', 'ave')
    assert final.all() and np.isfinite(d).mean() >= 0.95 and np.isfinite(d[:67, :67]).all() and not f.target[:67, :67].any()
    # with the default reach the same terrain has no pit edge
    d32 = F.oracle(F.far_pit(row_varying, None))
    assert d32.n_warn == 1 and len(d32.pit_i) == 0


def test_near_pit_drains_round_a_tile_corner():
    f = F.near_pit()
    o = oracle('near_pit')
    m = f.elev.shape[1]
    (pit, dst), = F.pit_edges_kept(o)
    assert divmod(pit, m) == (30, 30) and o.n_warn == 0
    blocks = set(zip((dst // m // F.T).tolist(), (dst % m // F.T).tolist()))
    assert (0, 0) not in blocks and len(blocks) == 3


# ---- the fields of the UCA sweep (tests/test_gpu_uca_fields.py)
CHAINS = SNAKES + ('tall_long', 'wide_long', 'tile_snake_wide')


@pytest.mark.parametrize('name', CHAINS)
def test_uca_along_the_chains_is_a_running_count(name):
    """every cell area is 2 * 3 and every edge weight 1: uca along a path is 6, 12, 18, ... exactly, whatever the order of
    the additions; and the taint reaches every cell of these fields (no cell is done)"""
    f = getattr(F, name)()
    o = oracle(name)
    assert f.name == name and (o.A[2] == 1.0).all()
    for p in f.facts['paths']:
        want = np.cumsum((o.dX2 * o.dY2)[p[:, 0]])
        assert np.array_equal(want, 6.0 * np.arange(1, len(p) + 1))
        assert np.array_equal(o.uca[p[:, 0], p[:, 1]], want)
    assert o.edge_done.sum() == 0


def test_the_long_chains_pass_the_capped_grids():
    assert F.tall_long().elev.shape == (16500, 3) and F.wide_long().elev.shape == (3, 16500)
    assert F.LONG > 16384 and -(-F.LONG // 256) > 64
    assert F.tall_long().facts['crossings'] == F.wide_long().facts['crossings'] == 515
    assert F.tall_long().facts['depth'] == F.wide_long().facts['depth'] == F.LONG
    # the wide tile snake: four whole blocks of columns and a ragged one, one crossing from block to block
    f = F.tile_snake_wide()
    assert f.elev.shape == (40, 134) and f.facts['crossings'] == 4 and f.facts['longest_run'] == 1024
    assert f.facts['depth'] == 32 * 134


@pytest.mark.parametrize('kl,kr', [(3, 0), (4, 7)])
def test_roofs_are_partly_tainted(kl, kr):
    f = F.roof(kl, kr)
    o = oracle('roof', kl, kr)
    n, m = f.elev.shape
    assert (n, m) == (70, 90) and f.name == 'roof%d%d' % (kl, kr)
    # one section per half, two unequal out-edges per cell, no edge across the ridge
    r = f.facts['ridge']
    assert np.array_equal(np.unique(o.section[:, :r]), [kl]) and np.array_equal(np.unique(o.section[:, r:]), [kr])
    od = F.out_degree(o)
    assert (od == 2).mean() >= 0.90 and np.array_equal(f.target, od < 2) and np.abs(o.A[2] - 0.5).min() > 0.05
    indptr, indices, _ = o.A
    src = np.repeat(np.arange(n * m), np.diff(indptr))
    assert ((src % m < r) == (indices % m < r)).all()
    # only one of the top and bottom rows takes flow from outside: the taint stops short of most of the grid
    todo, done = o.edge_todo.astype(bool), o.edge_done.astype(bool)
    assert todo.sum() == 88 and (todo[0].any() != todo[-1].any()) and not todo[1:-1].any()
    assert 0.4 <= done.mean() <= 0.8 and done.sum() == 4230
    mixed, total = F.blocks_mixed(done)
    assert total == 9 and mixed >= 5
    assert not np.isnan(o.uca).any()


@pytest.mark.parametrize('shape', [(16500, 5), (5, 16500)])
def test_strips_hold_pits_flats_and_every_section(shape):
    f = F.strip(shape)
    o = oracle('strip', shape)
    assert f.elev.shape == shape and f.name == 'strip_%dx%d' % shape and max(shape) > 16384
    assert len(np.unique(o.pit_i)) >= 100 and o.flats.any()
    assert set(range(8)) <= set(np.unique(o.section).tolist())
    assert 0.1 <= o.edge_done.astype(bool).mean() <= 0.9
