"""Host-side validation of the conv weight-gradient launchers under AddressSanitizer + UBSan.

Builds csrc/tests/wgrad_validation.cpp with csrc/kernels/conv_wgrad.hip and csrc/kernels/wino_wgrad.hip
(host code instrumented, device code unchanged) and runs the program on the CPU: missing or misaligned
operands, empty shapes (an empty batch used to divide by zero), a zero stride (likewise), a kernel
larger than the padded map, pixel counts past 32 bits, non-positive output strides and an unknown tile
config must be rejected by tp_conv_wgrad and tp_wino_wgrad before any GPU work."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_wgrad_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("wgrad_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wgrad validation ok" in r.stdout
