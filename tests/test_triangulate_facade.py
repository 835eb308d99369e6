"""The C++ façade sfm::Triangulator (include/sfm/triangulator.hpp) on a small
WorldStructure, checked inside tests/cpp/triangulate_test.cpp: the host build
(csrc/tri.cpp's host path compiled in, no library) on the CPU, the library
build with the GPU façade on the GPU."""
import os
import subprocess

import pytest

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def _run(exe, *args):
    path = os.path.join(CPP, exe)
    assert os.path.exists(path), "run make (builds the C++ triangulation tests)"
    r = subprocess.run([path, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triangulate ok" in r.stdout
    return r.stdout


def test_host_triangulator_standalone():
    assert "host:" in _run("triangulate_host_test")


def test_host_triangulator_through_the_library():
    assert "host:" in _run("triangulate_test")


@pytest.mark.gpu
def test_gpu_triangulator():
    assert "gpu: 39 points written" in _run("triangulate_test", "--gpu")
