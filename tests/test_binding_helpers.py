"""csrc/include/tp_bind.h holds the torch-side helpers of the two binding files (source text only:
nothing is built, no GPU).

bindings.cpp and engine_bindings.cpp once carried a ``cur_stream()`` and a ``TP_CHECK_HIP`` each
(with different messages) and their own copies of the operand checks, which drifted apart. Both are
now defined once, in the header that both files include; the kernel files must not see it (it pulls
in torch headers, and no torch type crosses the launcher boundary)."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "csrc"
HEADER = CSRC / "include" / "tp_bind.h"
BINDINGS = [CSRC / "bindings.cpp", CSRC / "engine_bindings.cpp"]
SOURCES = [f for f in sorted(CSRC.rglob("*")) if f.suffix in (".h", ".hip", ".cpp")]
INCLUDE = re.compile(r'^\s*#\s*include\s*[<"](?:[\w./]*/)?tp_bind\.h[>"]', re.M)


def definitions(pattern):
    return [f.relative_to(CSRC).as_posix() for f in SOURCES for _ in re.finditer(pattern, f.read_text(), re.M)]


def test_stream_and_launch_check_are_defined_once():
    assert len(SOURCES) > 20, "the source files are not found"
    # a definition: the name followed by a body, not a call ``cur_stream())``
    assert definitions(r"\bcur_stream\s*\(\s*\)\s*\{") == ["include/tp_bind.h"]
    assert definitions(r"^\s*#\s*define\s+TP_CHECK_HIP\b") == ["include/tp_bind.h"]
    assert '"tpamd kernel launch failed: "' in HEADER.read_text()


def test_both_binding_files_include_the_header():
    for f in BINDINGS:
        assert INCLUDE.search(f.read_text()), f.relative_to(CSRC)


def test_header_is_part_of_the_source_stamp():
    """an edit of the header must rebuild both bindings: the build hashes every csrc/include/*.h
    into each object's digest and into the stamp that ops.load() checks"""
    from torchpruner_amd import _build
    headers, _, bindings = _build._sources()
    assert HEADER in headers and sorted(bindings) == sorted(BINDINGS)


def test_no_kernel_file_includes_the_header():
    kernels = sorted((CSRC / "kernels").glob("*.hip"))
    assert len(kernels) >= 17
    # nor any other header or host validation program: only the two binding files
    for f in SOURCES:
        if f != HEADER and f not in BINDINGS:
            assert not INCLUDE.search(f.read_text()), f.relative_to(CSRC)
