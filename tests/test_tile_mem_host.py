"""The ownership layer of a tile's device memory (csrc/tile_mem.h: tile_alloc, tile_reserve, tile_release_all, dev_reserve)
on the host: tests/host/tile_mem_check.cpp supplies malloc-backed fakes of plane_take / plane_give / dev_malloc / dev_free,
runs a scripted sequence of calls with every allocation failing once, and is built and run here as a stand-alone program under
the address and undefined-behaviour sanitizers.  No GPU, no library loaded into this process."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def test_tile_mem_check(tmp_path):
    from pydem_amd.build import HIPCC
    exe = str(tmp_path / 'tile_mem_check')
    src = os.path.join(ROOT, 'tests', 'host', 'tile_mem_check.cpp')
    # host code only: the sanitizers are named for the host side alone
    cc = subprocess.run([HIPCC, '-x', 'hip', '--offload-host-only', '-std=c++17', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined', src, '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].startswith('tile_mem_check: ok'), run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr
