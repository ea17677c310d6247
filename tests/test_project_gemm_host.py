"""Host-side validation of the project GEMM launchers under AddressSanitizer + UBSan.

Builds csrc/tests/project_gemm_validation.cpp with csrc/kernels/scaled_project.hip, silu_project.hip and
silu_prefix_project.hip (host code instrumented, device code unchanged) and runs the program on the CPU:
tp_scaled_project, tp_silu_project_fwd, tp_silu_project_dgrad and tp_silu_prefix_project must reject missing
or misaligned operands, empty shapes, widths that are no multiple of 4 (or above 128), rows that are not
B * HW, a prefix range outside the permutation, a wrong slot count or tay_mode and operands of 2^31 bytes or
more before any GPU work, with no overflow in the size products; tp_silu_project_tay_slots must equal a
brute-force count of the 64-row tiles an image meets. The Python twin of that formula is checked here against
the same count."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_project_gemm_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("project_gemm_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "project_gemm validation ok" in r.stdout


def test_tay_slots_is_the_most_tiles_an_image_meets():
    """Image b of hw rows holds rows b hw .. (b + 1) hw - 1; b hw mod 64 has a period of at most 64."""
    from torchpruner_amd import ops
    for hw in range(1, 301):
        most = max(((b + 1) * hw - 1) // 64 - (b * hw) // 64 + 1 for b in range(64))
        for C in (4, 64, 132):
            assert ops.silu_project_tay_slots(hw, C) == most, (hw, C)
    for hw, C in ((0, 8), (-64, 8), (64, 0), (64, -8), (64, 2), (64, 30)):
        assert ops.silu_project_tay_slots(hw, C) == 0
