"""Host-side validation of the elementwise launchers under AddressSanitizer + UBSan.

Builds csrc/tests/elementwise_validation.cpp with channel_reduce.hip, prune_ops.hip, shapley.hip,
train_ops.hip and data_ops.hip (host code instrumented, device code unchanged) and runs the program
on the CPU: null pointers, non-positive sizes, unknown modes, impossible pool geometries (a stride
of 0 included), batches past the grid limits, operands whose 32-bit index math would overflow,
dropout probabilities outside [0, 1) and misaligned dropout operands must be rejected before any
GPU work; zero-work calls succeed; the reduction workspace covers both NHWC kernels; the dropout
generator reproduces its Philox4x32-10 vectors on the host."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_elementwise_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("elementwise_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "elementwise validation ok" in r.stdout
