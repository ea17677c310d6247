"""Host-side validation of the nine-product 2x2-map conv launchers under AddressSanitizer + UBSan.

Builds csrc/tests/conv2x2_fast_validation.cpp with csrc/kernels/conv2x2_fast.hip and conv_mfma.hip
(host code instrumented, device code unchanged) and runs the program on the CPU: channel counts off
the K-slice / float4 granules, empty shapes, unknown tile configs, split counts that are not
normalised, operands of 2^31 bytes or more and missing or misaligned operands must be rejected
before any GPU work."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_conv2x2_fast_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("conv2x2_fast_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "conv2x2_fast validation ok" in r.stdout
