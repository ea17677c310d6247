"""csrc/include/tp_launchers.h is the only place a C launcher is declared (source text only: nothing
is built, no GPU).

A launcher is an ``extern "C"`` function of 10 to 33 positional arguments; a caller compiled against a
stale hand-copied prototype still links and then passes pointers in the wrong slots. So every
launcher defined in csrc/kernels/*.hip is declared exactly once in the header, nothing else under
csrc/ declares one, and every kernel file and host validation program includes the header: a
definition or a call that disagrees with the declaration then fails to compile."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "csrc"
HEADER = CSRC / "include" / "tp_launchers.h"
KERNELS = sorted((CSRC / "kernels").glob("*.hip"))

# extern "C" <type> tp_name(<args>) followed by a body
DEFINITION = re.compile(r'^extern "C" [\w ]+?[ *](tp_\w+)\([^;{]*\)\s*\{', re.M)
# a prototype: extern "C" <type> name(<args>);  (a braced extern "C" { ... } block is matched apart)
PROTOTYPE = re.compile(r'^extern "C" [^;{(]*\([^;{]*\)\s*;', re.M)
BLOCK = re.compile(r'^extern "C" \{', re.M)


def defined_launchers():
    names = []
    for k in KERNELS:
        names += DEFINITION.findall(k.read_text())
    return names


def test_every_launcher_is_declared_exactly_once():
    names = defined_launchers()
    assert len(names) > len(KERNELS), "the pattern no longer finds the definitions"
    assert len(set(names)) == len(names), "a launcher is defined twice"
    header = HEADER.read_text()
    for name in names:
        # a declaration starts its line with the return type; comments that mention the name do not count
        decls = re.findall(r'^(?!\s*//)[\w ]+?[ *]%s\([^;{]*\);' % re.escape(name), header, re.M)
        assert len(decls) == 1, f"{name}: {len(decls)} declarations in {HEADER.name}"
    declared = re.findall(r'^(?!\s*//)[\w ]+?[ *](tp_\w+)\([^;{]*\);', header, re.M)
    assert sorted(declared) == sorted(names), set(declared) ^ set(names)


def test_no_other_file_declares_a_launcher():
    for f in sorted(CSRC.rglob("*")):
        if f == HEADER or f.suffix not in (".h", ".hip", ".cpp"):
            continue
        text = f.read_text()
        assert not PROTOTYPE.search(text), f"{f.relative_to(CSRC)} declares an extern \"C\" function itself"
        assert not BLOCK.search(text), f"{f.relative_to(CSRC)} has an extern \"C\" block of its own"


def test_kernels_and_host_programs_include_the_header():
    tests = sorted((CSRC / "tests").glob("*.cpp"))
    assert len(KERNELS) >= 17 and len(tests) >= 8
    for f in KERNELS + tests:
        assert re.search(r'^#include "tp_launchers\.h"$', f.read_text(), re.M), f.relative_to(CSRC)
