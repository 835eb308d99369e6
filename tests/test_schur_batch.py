"""[cpu] The Schur kernel's batch rule (csrc/ba_types.h batch_fits /
batch_count, which the kernel's batch_points takes by ballot) walked on the
host for every batch shape the kernels are built with: no batch above the
point or observation cap, the longest batch that fits, progress for every
track of 1 .. cap, the empty batch for cap + 1 (tests/cpp/batch_points_test.cpp,
built by the Makefile)."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "batch_points_test")


def test_batch_rule_caps_and_progress():
    assert os.path.exists(EXE), "run make (builds tests/cpp/batch_points_test)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batches walked, 0 bad" in r.stdout
