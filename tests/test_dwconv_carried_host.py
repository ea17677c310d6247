"""Host-side validation of the carried-width depthwise-conv launchers and of the BatchNorm
launchers' activation code under AddressSanitizer + UBSan.

Builds csrc/tests/dwconv_carried_validation.cpp with csrc/kernels/dwconv.hip and batchnorm.hip
(host code instrumented, device code unchanged) and runs the program on the CPU: a parameter
width Cw <= 0 or > C, Cw < C at a C that is no multiple of 4, misaligned pointers and the grid and
2 GiB limits must be rejected by tp_dwconv_{fwd,dgrad,wgrad} before any GPU work, and the
BatchNorm forward launchers must reject an activation code outside 0..2 (and ReLU6 without a mask)."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_dwconv_carried_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("dwconv_carried_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dwconv carried validation ok" in r.stdout
