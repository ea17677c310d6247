"""Host-side validation of the LDS-staged SiLU depthwise-conv launchers under AddressSanitizer + UBSan.

Builds csrc/tests/dwconv_silu_validation.cpp with csrc/kernels/dwconv_silu.hip (host code instrumented,
device code unchanged) and runs the stand-alone program on the CPU: unsupported geometries, activation
codes other than 0 | 4 / 4, channel counts that are no multiple of 4, empty outputs, missing or
misaligned operands (`pre`, `apoz`, `pool` and `tay` included), operands of 2^31 bytes or more, a
partial slab of another slot count and a bad tay_mode must be rejected before any GPU work; the tile
of every map up to 130 x 130 covers the map, fits the slab and the LDS."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_dwconv_silu_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("dwconv_silu_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dwconv_silu validation ok" in r.stdout
