"""Host-side validation of the Hardswish-aware depthwise-conv launchers under AddressSanitizer + UBSan.

Builds csrc/tests/dwconv_hs_validation.cpp with csrc/kernels/dwconv_act.hip (host code instrumented,
device code unchanged) and runs the stand-alone program on the CPU: unsupported geometries,
activation codes outside 0..3, channel counts that are no multiple of 4, empty outputs, missing or
misaligned operands (`pre` included), a missing y when out_act != 0, operands of 2^31 bytes or more
and a partial slab of another slot count must be rejected before any GPU work."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_dwconv_hs_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("dwconv_hs_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dwconv_hs validation ok" in r.stdout
