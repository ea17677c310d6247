"""Host-side validation of the fused BatchNorm + Hardswish launchers under AddressSanitizer + UBSan.

Builds csrc/tests/bn_hswish_validation.cpp with csrc/kernels/batchnorm.hip (host code instrumented,
device code unchanged) into a stand-alone executable and runs it on the CPU: non-positive sizes,
more parameter channels than the activation carries, activations of 2^32 elements or more and (in
the backward) missing affine rows must be rejected before any pointer is touched."""
import os
import subprocess

import pytest


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_bn_hswish_validation_asan():
    from torchpruner_amd._build import build_host_program
    exe = build_host_program("bn_hswish_validation")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bn hswish validation ok" in r.stdout
