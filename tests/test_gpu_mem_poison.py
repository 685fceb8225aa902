"""GPU tier: no result depends on what handed-out device memory held.

Every device block the library hands out comes through three doors of csrc/devmem.hip -- plane_take (the free lists of
destroyed tiles' planes), dev_malloc, and the conditioning arena at the start of a lease -- and holds "whatever the last owner
left".  With PYDEM_MEM_POISON=<byte> each door fills the block with that byte first.  The scenarios of tests/mem_poison_kit.py
(the per-tile pipeline, an edge round, the flow-graph analyses, fill and depressions, a seam session, the mosaics, the regrown
tile, a tile on the planes of the tile before) run once per mode in a child process of their own -- four children, one at a
time, each cached -- and ship sha256 digests of their outputs:

  unset   what hipMalloc returns in a young process (often zeros) and what earlier scenarios left;
  0x00    zeros everywhere: a kernel that needs a zeroed counter passes here and only here;
  0xFF    NaN doubles, -1 integers, every flag bit set;
  0x7F    huge finite doubles, large positive integers: a stale read that a NaN comparison drops silently still shows.

Bars: every output has the same bytes in all four modes (test_same_bytes_in_every_mode: a failure names scenario, mode and
output); in the unset child every scenario is also held to the host reference of its own GPU test, comparator and tolerance
imported from there (test_unset_run_matches_its_reference); the hook ran where it should and nowhere else (test_coverage).

Time: the unset child, which also computes every host reference, spent 4.2 s in its scenarios on an MI355X when this was
written, a poisoned child (the device paths only, a device synchronisation and a fill per hand-out) 3.0 s; with the start of
python and of the HIP runtime a child is over in about 10 s.  CHILD_TIMEOUT is a wide margin over that."""
import json

import pytest

import mem_poison_kit as K
from flowgraph_kit import run_child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300
POISONED = [m for m in K.MODES if m != 'unset']
_CHILDREN = {}


def child(mode):
    """The result of the child of `mode`, started once: a child that failed is not started again."""
    if mode not in _CHILDREN:
        value = K.MODES[mode]
        body = "\n".join(["import os",
                          "os.environ.pop('PYDEM_MEM_POISON', None)" if value is None else "os.environ['PYDEM_MEM_POISON'] = %r" % value,
                          "import mem_poison_kit",
                          "mem_poison_kit.main(anchor=%r)" % (value is None)])
        try:
            r = run_child(body, timeout=CHILD_TIMEOUT)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith(K.RESULT_TAG)][-1]
            _CHILDREN[mode] = json.loads(line[len(K.RESULT_TAG):])
        except Exception as e:              # (also a timeout: every test of the mode reports it, none repeats it)
            _CHILDREN[mode] = e
    if isinstance(_CHILDREN[mode], Exception):
        raise AssertionError("the child of mode %s did not finish: %r" % (mode, _CHILDREN[mode]))
    return _CHILDREN[mode]


def scenario(mode, name):
    rec = child(mode)['scenarios'][name]
    assert 'error' not in rec, "%s in mode %s:\n%s" % (name, mode, rec.get('error'))
    return rec


@pytest.mark.parametrize('name', K.NAMES)
def test_unset_run_matches_its_reference(name):
    rec = scenario('unset', name)
    assert rec['digests'], name
    assert rec['anchor'] is None, "%s against its host reference (variable unset):\n%s" % (name, rec['anchor'])


@pytest.mark.parametrize('mode', POISONED)
@pytest.mark.parametrize('name', K.NAMES)
def test_same_bytes_in_every_mode(name, mode):
    want, got = scenario('unset', name)['digests'], scenario(mode, name)['digests']
    assert sorted(got) == sorted(want), (name, mode)
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, "%s: with device memory handed out as %s these outputs differ from the run with the variable unset: %s" % (name, mode, differ)


@pytest.mark.parametrize('mode', list(K.MODES))
def test_coverage(mode):
    res = child(mode)
    if mode == 'unset':
        assert res['mode'] is None and res['stats_start'] == [0, 0] and res['stats_end'] == [0, 0]
        assert all(rec.get('stats_after', [0, 0]) == [0, 0] for rec in res['scenarios'].values())
        return
    assert res['mode'] == K.MODES[mode] and res['stats_start'] == [0, 0]
    # every block in the regrown tile's registry came through a poisoned door (blocks that regrew count twice)
    scenario(mode, 'tile_memory')
    tm = res['extra']['tile_memory']
    assert tm['device_bytes'] > 0 and tm['poisoned_bytes'] >= tm['device_bytes'], tm
    # ... and every scenario took device memory
    for name in K.NAMES:
        rec = scenario(mode, name)
        assert rec['stats_after'][0] > rec['stats_before'][0] and rec['stats_after'][1] > rec['stats_before'][1], (name, rec)
