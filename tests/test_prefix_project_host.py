"""Host-side validation of the prefix-scan project-conv launcher under AddressSanitizer + UBSan.

Builds csrc/tests/prefix_project_validation.cpp with csrc/kernels/prefix_project.hip (host code
instrumented, device code unchanged) and runs the program on the CPU: an output width that is no
multiple of 4, empty shapes, a prefix range outside the permutation (cnt < 1, p0 < 0,
p0 + cnt - 1 > n, n > C), missing or misaligned operands and operands of 2^31 bytes or more must be
rejected before any GPU work."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_prefix_project_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("prefix_project_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prefix_project validation ok" in r.stdout
