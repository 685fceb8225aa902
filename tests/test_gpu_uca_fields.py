"""The UCA sweep (csrc/uca.hip K5: k_sweep_tiles, k_sweep_tiles_listed, k_sweep_tiles_resident; csrc/uca_sym.inl: k_sweep_sym,
k_sym_finish; plain and weighted) on the designed fields of tests/flow_fields.py, cell by cell against the CPU oracle.

The fields: every one of tests/test_gpu_flow_fields.py (the snakes, the sixteen fans, the pits, tall and wide), and those made
for the sweep, which tests/test_flow_fields.py pins on the CPU: two roofs (the edge taint covers part of the grid and part of
most 32-blocks), a tile snake with wholly open tiles at the pass after the two full ones, chains and fractal strips with a side
of 16500 (past the 16384 rows and the 64 x 256 columns of the capped launches of the row, column and line-gather kernels).

Per field, after the precondition that the device's edge set is the oracle's:
  uca within the bar of tests/test_gpu_parity.py (_close), edge_todo and edge_done bit for bit; on the strips every field of
    the full path (mag, direction, flats, section, proportion, twi) and the line gathers of both axes;
  on the chains uca == 6, 12, 18, ... along every path, exactly (each cell area is 2 * 3, each edge weight 1: every partial
    sum is a small integer, whatever the order and whether a visit adds numbers or composes coefficients);
  a fan and its mirror image give column-reversed results;
  calc_weighted_uca(1) is uca bit for bit, random weights (scaled by the cell area and not) are within BOUND of the weighted
    reference of tests/test_gpu_weighted_uca.py, and uca and the masks are as they were afterwards.

The schedule switches are read once per process: every schedule runs all fields in one child process (one at a time) against
references the parent computes once.  The PYDEM_SWEEP_DEBUG lines of each sweep show that the schedule took its branch.
Schedules are not compared with one another: a numeric, a resident and a symbolic visit add a cell's in-edges in different
orders.  For the same reason w = 1 gives uca's bits only while the weighted sweep follows the plain sweep's schedule: under
PYDEM_SWEEP_FIRST=lds and PYDEM_SWEEP_DENSE, which the weighted sweep used to ignore, 53 cells of near_pit differed in their
last bits until K5a and K5d got weighted instantiations."""
import collections
import functools
import os
import pickle
import re
import shutil
import sys
import warnings

import numpy as np
import pytest

import flow_fields as F
from flowgraph_kit import assert_bound, assert_same_bits, random_weights, run_child
from test_gpu_flow_fields import FIELDS as FLOW_FIELDS, processor

pytestmark = pytest.mark.gpu

STRIPS = ('strip_16500x5', 'strip_5x16500')
CHAINS = ('row_snake', 'tile_snake', 'tall', 'wide', 'tall_long', 'wide_long', 'tile_snake_wide')
FIELDS = dict(list(FLOW_FIELDS.items())
              + [('roof30', functools.partial(F.roof, 3, 0)), ('roof47', functools.partial(F.roof, 4, 7)),
                 ('tile_snake_wide', F.tile_snake_wide), ('tall_long', F.tall_long), ('wide_long', F.wide_long),
                 (STRIPS[0], functools.partial(F.strip, (16500, 5))), (STRIPS[1], functools.partial(F.strip, (5, 16500)))])
WEIGHT_SEED = 7
MIRROR_BOUND, MIRROR_FLOOR = 1e-9, 1e-300          # those of test_gpu_flow_fields.test_fans_agree_with_their_mirror_image
RECORD = ('row_snake', 'tile_snake', 'tile_snake_wide', 'far_pit', 'tall_long')      # fields whose counts are printed

SCHEDULES = [('default', {}),
             ('numeric', {'PYDEM_SWEEP_SYM': '0'}),
             ('numeric_generic', {'PYDEM_SWEEP_SYM': '0', 'PYDEM_SWEEP_RESIDENT': '0'}),
             ('symbolic_at_2_generic', {'PYDEM_SWEEP_SYM': '2', 'PYDEM_SWEEP_RESIDENT': '0'}),
             ('lds_first', {'PYDEM_SWEEP_FIRST': 'lds'}),
             ('dense_3', {'PYDEM_SWEEP_DENSE': '3'})]


# ---- the references: once, in the parent
@pytest.fixture(scope='module')
def references(tmp_path_factory):
    """a directory with one file per field: the oracle after calc_uca (after calc_twi on the strips) and the weighted references
    for the random weights, scaled by the cell area and not: (reference of w, reference of |w|)"""
    from test_gpu_weighted_uca import weighted_ref
    d = str(tmp_path_factory.mktemp('uca_fields'))
    for name, make in FIELDS.items():
        field = make()
        assert field.name == name, (field.name, name)
        o = F.oracle(field)
        if name in STRIPS:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                o.calc_twi()
        w = random_weights(field.elev.shape, WEIGHT_SEED)
        weighted = {scale: (weighted_ref(o, w, scale), weighted_ref(o, np.abs(w), scale)) for scale in (True, False)}
        with open(os.path.join(d, name + '.pkl'), 'wb') as fh:
            pickle.dump(dict(o=o, weighted=weighted), fh, pickle.HIGHEST_PROTOCOL)
    yield d
    shutil.rmtree(d, ignore_errors=True)


# ---- the child: every field on the device
def _mark(name, what):
    sys.stderr.write('--- %s %s\n' % (name, what))
    sys.stderr.flush()


def _fresh(dp, *names):
    """the fields as the device holds them now, not as the host remembers them"""
    for k in names:
        dp._host.pop(k, None)
    return [np.array(getattr(dp, k)) for k in names]


def check_lines(dp, names):
    """get_line and get_lines of the first and last row and column against the downloads"""
    n, m = dp.shape
    full = dict(zip(names, _fresh(dp, *names)))
    requests = [(k, axis, index) for k in names for axis, index in ((1, 0), (1, m - 1), (0, 0), (0, n - 1))]
    for k in names:
        dp._host.pop(k, None)
    assert all(k in dp._on_device for k in names)
    both = dp.get_lines(requests)
    for (k, axis, index), line in zip(requests, both):
        want = full[k][index, :] if axis == 0 else full[k][:, index]
        one = dp.get_line(k, axis, index)
        assert one.shape == line.shape == want.shape == ((m,) if axis == 0 else (n,))
        nan_ok = want.dtype.kind == 'f'
        assert np.array_equal(one, want, equal_nan=nan_ok), "get_line(%r, %d, %d)" % (k, axis, index)
        assert np.array_equal(line, want, equal_nan=nan_ok), "get_lines: (%r, %d, %d)" % (k, axis, index)
    return len(requests)


def child(d):
    """(child process) every field against its references in the directory d; prints {field: tile passes of calc_uca}"""
    from test_gpu_parity import _close, assert_edge_set_equals_oracle
    from test_gpu_scale_paths import check_full_path
    from test_gpu_weighted_uca import BOUND
    passes, fans = {}, {}
    for name, make in FIELDS.items():
        field = make()
        with open(os.path.join(d, name + '.pkl'), 'rb') as fh:
            ref = pickle.load(fh)
        o = ref['o']
        _mark(name, 'uca %d' % int(o.stats[0]))
        dp = processor(field)
        passes[name] = int(dp.timings['sweep_tile_passes'])
        _mark(name, 'checks')
        assert_edge_set_equals_oracle(o, dp)
        uca, todo, done = (np.array(x) for x in (dp.uca, dp.edge_todo, dp.edge_done))
        _close(uca, o.uca, name + ': uca')
        assert np.array_equal(todo, o.edge_todo), "%s: edge_todo differs in %d cells" % (name, (todo != o.edge_todo).sum())
        assert np.array_equal(done, o.edge_done), "%s: edge_done differs in %d cells" % (name, (done != o.edge_done).sum())
        if name in CHAINS:
            for p in field.facts['paths']:
                want = np.cumsum((o.dX2 * o.dY2)[p[:, 0]])
                got = uca[p[:, 0], p[:, 1]]
                assert np.array_equal(got, want), "%s: %d cells of a chain of %d are not 6 k" % (name, (got != want).sum(), len(p))
        if name.startswith('fan'):
            if name.endswith('_mirror'):
                a, at, ad = fans[name[:-len('_mirror')]]
                assert_bound(a, uca[:, ::-1], o.uca[:, ::-1], name[:-len('_mirror')] + ' against its mirror image', MIRROR_BOUND, MIRROR_FLOOR)
                assert np.array_equal(at, todo[:, ::-1]) and np.array_equal(ad, done[:, ::-1]), name
            else:
                fans[name] = (uca, todo, done)
        # the weighted instantiations
        _mark(name, 'weighted')
        w = random_weights(field.elev.shape, WEIGHT_SEED)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert_same_bits(dp.calc_weighted_uca(1.0), uca, name + ': w = 1')
            for scale in (True, False):
                want, scale_abs = ref['weighted'][scale]
                got = np.array(dp.calc_weighted_uca(w, scale_by_cell_area=scale))
                assert_bound(got, want, scale_abs, '%s: random weights%s' % (name, '' if scale else ', unscaled'), BOUND)
        _mark(name, 'after')
        uca2, todo2, done2 = _fresh(dp, 'uca', 'edge_todo', 'edge_done')
        assert_same_bits(uca2, uca, name + ': uca after the weighted calls')
        assert np.array_equal(todo2, todo) and np.array_equal(done2, done), name + ': masks after the weighted calls'
        assert int(dp.timings['sweep_tile_passes']) == passes[name]
        if name in STRIPS:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                twi = dp.calc_twi()
            check_full_path(dp, o, twi)
            assert check_lines(dp, ('uca', 'edge_done', 'section')) == 12
        del dp
    assert len(fans) == 8
    print('RESULTS', passes)


# ---- the debug lines of one child
Sweep = collections.namedtuple('Sweep', 'first listed looks_before symbolic looks_after two_level circular')


def sweeps_of(block):
    """The sweeps a block of PYDEM_SWEEP_DEBUG lines reports, one per "tile passes a-b" line: the two full passes (their numbers),
    the tiles they list, the host's looks (pass, listed next, passes per look, kind of visit) before the symbolic pass and after
    it, the symbolic pass (pass, listed next) and the counters of the two-level solve (symbolic tiles, fall-backs, pool used, pool)"""
    out, cur = [], None
    for line in block.splitlines():
        mt = re.match(r'tile passes (\d+)-(\d+): \d+ cells of \d+, (\d+) tiles listed$', line)
        if mt:
            cur = dict(first=(int(mt.group(1)), int(mt.group(2))), listed=int(mt.group(3)), looks_before=[], symbolic=None,
                       looks_after=[], two_level=None, circular=False)
            out.append(cur)
            continue
        if cur is None:
            continue
        mt = re.match(r'listed tile pass (\d+): (\d+) tiles listed next, processed \d+ \((\d+) (resident|generic) passes\)$', line)
        if mt:
            look = (int(mt.group(1)), int(mt.group(2)), int(mt.group(3)), mt.group(4))
            cur['looks_before' if cur['symbolic'] is None else 'looks_after'].append(look)
        mt = re.match(r'symbolic pass (\d+): \d+ cells of \d+, (\d+) tiles listed$', line)
        if mt:
            assert cur['symbolic'] is None, block
            cur['symbolic'] = (int(mt.group(1)), int(mt.group(2)))
        mt = re.match(r'two-level solve: (\d+) symbolic tiles \((\d+) fell back to numeric visits\), \d+ outlets, \d+ symbolic cells, '
                      r'pool (\d+) of (\d+) doubles', line)
        if mt:
            cur['two_level'] = tuple(int(x) for x in mt.groups())
        if line.startswith('circular drainage') or line.startswith('pydem: circular drainage'):
            cur['circular'] = True
    return [Sweep(**s) for s in out]


def check_sweep(env, S, what):
    """the branches one sweep took against what the switches ask for (csrc/uca.hip stage_sweep).  Every field here has fewer
    than 4096 tiles, so the default switches mean: the symbolic pass right after the two full passes, resident visits."""
    sym = int(env.get('PYDEM_SWEEP_SYM', 4096))
    kind = 'resident' if int(env.get('PYDEM_SWEEP_RESIDENT', 4096)) > 0 else 'generic'
    dense = int(env.get('PYDEM_SWEEP_DENSE', 0))               # (the weighted sweep follows the same schedule as the plain one)
    assert S.first == (dense + 1, dense + 2), (what, S)
    assert all(lk[3] == kind for lk in S.looks_before + S.looks_after), (what, kind, S)
    if sym == 0:
        # numeric visits to the end: listed passes until a look finds no tile listed
        assert S.symbolic is None and S.two_level is None and not S.looks_after, (what, S)
        assert bool(S.looks_before) == (S.listed > 0), (what, S)
        assert not S.looks_before or S.looks_before[-1][1] == 0, (what, S)
        return
    assert S.two_level is not None, (what, S)
    assert S.two_level[2] <= S.two_level[3], (what, S)
    # numeric listed passes while more than `sym` tiles are listed, then one symbolic visit of every open tile, then listed
    # passes (light visits) until no tile is listed
    assert bool(S.looks_before) == (S.listed > sym), (what, S)
    left = S.looks_before[-1][1] if S.looks_before else S.listed
    assert left <= sym and (S.symbolic is not None) == (left > 0), (what, S)
    if S.symbolic is None:
        assert not S.looks_after, (what, S)
    else:
        assert bool(S.looks_after) == (S.symbolic[1] > 0), (what, S)
        assert not S.looks_after or S.looks_after[-1][1] == 0, (what, S)


@pytest.mark.parametrize('schedule,env', SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_uca_on_the_designed_fields(references, schedule, env):
    """Every field in one child under the schedule (child() holds it to the oracle, the closed form, the mirror images and the
    weighted references), then the schedule's debug lines.

    The bound on the passes of the chains under PYDEM_SWEEP_SYM=0: a pass visits a tile at most once (k_sweep_tiles takes each
    tile id once from its band counter; the list of a listed pass holds a tile once, the stamp in N.flag sees to it), so a
    chain that alternates between two tiles advances at most two of its segments per pass and needs crossings // 2 - 1 passes
    or more.  The listing rule of csrc/uca.hip is stricter than the argument needs: tile_stage takes a neighbour's cell as
    final only if its level is below the pass (final_before: lv >= 1 && lv < pass), and a visit wakes its neighbours for the
    next pass, so a chain advances ONE segment per pass; the bound holds with that much room, and the passes are printed."""
    r = run_child("from test_gpu_uca_fields import child\nchild(%r)\nprint('CHILD-OK')" % references,
                  env=dict(env, PYDEM_SWEEP_DEBUG='1'), timeout=300)
    passes = eval(r.stdout.split('RESULTS', 1)[1].splitlines()[0])
    assert sorted(passes) == sorted(FIELDS)
    blocks = {}
    for block in r.stderr.split('--- ')[1:]:
        head, _, body = block.partition('\n')
        name, what = head.split(' ', 1)
        blocks[name, what.split(' ')[0]] = (body, what)
    numeric = env.get('PYDEM_SWEEP_SYM') == '0'
    if numeric:
        assert 'symbolic pass' not in r.stderr and 'two-level solve' not in r.stderr
    for name in FIELDS:
        body, what = blocks[name, 'uca']
        (S,) = sweeps_of(body)
        check_sweep(env, S, '%s, %s' % (name, schedule))
        if int(what.split(' ')[1]) <= 1:            # the oracle finished the field without re-seeding: so must the tile passes
            assert not S.circular, (name, body[-2000:])
        weighted = sweeps_of(blocks[name, 'weighted'][0])
        assert len(weighted) == 3, (name, len(weighted))
        for k, W in enumerate(weighted):
            check_sweep(env, W, '%s, %s, weighted call %d' % (name, schedule, k))
        assert not sweeps_of(blocks[name, 'after'][0])                # (downloads, twi and line gathers sweep nothing)
        if name in RECORD:
            print('%s, %s: %d tile passes, %d tiles listed after the full passes; %d looks before the symbolic pass, the last (pass, '
                  'listed next, passes per look, visits) %s; symbolic pass (pass, listed next) %s, then %d looks, the last %s; two-level '
                  'solve (symbolic tiles, fall-backs, pool used, pool) %s'
                  % (schedule, name, passes[name], S.listed, len(S.looks_before), S.looks_before[-1:], S.symbolic, len(S.looks_after),
                     S.looks_after[-1:], S.two_level))
    if not numeric:
        # the long chains still list tiles after the full passes (and three dense levels): a symbolic pass finishes them
        for name in ('row_snake', 'tile_snake_wide', 'tall', 'tall_long', 'wide_long'):
            assert sweeps_of(blocks[name, 'uca'][0])[0].symbolic is not None, name
    else:
        for name in ('row_snake', 'tall', 'tall_long'):
            crossings = FIELDS[name]().facts['crossings']
            assert passes[name] >= crossings // 2 - 1, (name, passes[name], crossings)
