"""Host-side validation of the squeeze-and-excitation launchers under AddressSanitizer + UBSan.

Builds csrc/tests/se_validation.cpp with csrc/kernels/squeeze_excite.hip (host code instrumented,
device code unchanged) and runs the program on the CPU: null pointers, non-positive sizes,
misaligned pointers on the float4 path, operands of 2^31 bytes or more and grids past the launch
limits must be rejected before any GPU work, and the split helper must stay in range."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_se_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("se_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "se validation ok" in r.stdout
