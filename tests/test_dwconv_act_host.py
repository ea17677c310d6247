"""Host-side validation of the fused depthwise-conv launchers under AddressSanitizer + UBSan.

Builds csrc/tests/dwconv_act_validation.cpp with csrc/kernels/dwconv_act.hip (host code
instrumented, device code unchanged) and runs the program on the CPU: unsupported geometries and
activation codes, channel counts that are no multiple of 4, empty outputs, missing or misaligned
operands, operands of 2^31 bytes or more and a partial slab of another slot count must be rejected
before any GPU work, and the slot helper must stay in range."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_dwconv_act_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("dwconv_act_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dwconv_act validation ok" in r.stdout
