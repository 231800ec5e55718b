"""The wave map of the 256 x 256-tile GEMM (csrc/gemm_edge.h) on the host: tests/cpp/gemm_edge_check.cpp walks every live extent
(lr, lc) in [1, 256]^2 of a block tile and checks that the map is a permutation of the eight 128 x 64 sub-tiles, that a wave is live
exactly when its sub-tile intersects lr x lc, that a full tile keeps the plain map (wave >> 2, wave & 3), that with at most four live
sub-tiles they sit on waves 0 .. nl - 1 with no two on one SIMD (wave & 3), and that with more than four the map is the plain one.
No GPU: the header is plain constexpr arithmetic, compiled here by the host compiler."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


def test_wave_map_at_every_live_extent(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'gemm_edge_check')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(PKG, 'csrc'),
                            os.path.join(ROOT, 'tests', 'cpp', 'gemm_edge_check.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert '65536 extents, 0 failures' in run.stdout
