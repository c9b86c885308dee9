"""What the tests of the C ABI share: the loaded library as a fixture, and the prototypes of a header under include/ as ctypes
types, for tests/test_abi_surfaces.py to hold against `_native.ABI_SURFACES`.  Imported by bare name; CPU only."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
CSRC = ROOT / "audio_cut_amd" / "csrc"

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "long long": C.c_int64, "float": C.c_float, "double": C.c_double}


@pytest.fixture(scope="session")
def lib():
    """libaudiocut_hip.so, built first where it is missing, with every signature declared and every header's version checked."""
    from audio_cut_amd import _native
    if not _native.library_path().exists():
        subprocess.run(["make", "-C", str(CSRC)], check=True)
    return _native.load()


def code(header: str) -> str:
    """The header without its comments."""
    text = re.sub(r"/\*.*?\*/", " ", (INCLUDE / header).read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _c_type(decl: str, named: bool) -> str:
    """'const float* x' -> 'float*', 'ac_ctx** out' -> 'ac_ctx**', 'int64_t n' -> 'int64_t'."""
    assert re.fullmatch(r"[\w\s*]+", decl), f"cannot read the type of {decl!r}"
    tokens = re.findall(r"\w+|\*", decl)
    if named and len(tokens) > 1 and tokens[-1] != "*":
        tokens = tokens[:-1]                                           # the parameter's name
    return " ".join(t for t in tokens if t not in ("*", "const")) + "*" * tokens.count("*")


def prototypes(header: str) -> list:
    """[(return type, name, [parameter types])] of every `ac_*` function the header declares, as C type names without `const`
    and without parameter names.  A declaration this cannot read is an error, never a gap in the list."""
    text = re.sub(r"^\s*#[^\n]*", " ", code(header), flags=re.M).replace('extern "C" {', " ").replace("}", " ")
    out = []
    for statement in (" ".join(s.split()) for s in text.split(";")):
        if not statement or re.fullmatch(r"typedef struct \w+ \w+", statement):
            continue
        m = re.fullmatch(r"(.+?)\b(ac_[a-z0-9_]+) ?\(([^()]*)\)", statement)
        assert m, f"{header}: cannot read the declaration {statement!r}"
        params = [] if m.group(3).strip() == "void" else [_c_type(p, named=True) for p in m.group(3).split(",")]
        out.append((_c_type(m.group(1), named=False), m.group(2), params))
    return out


def ctype(c_type: str, is_return: bool = False):
    """The ctypes type the binding must declare for a C type of the headers; an unknown type is an error."""
    if c_type in SCALARS:
        return SCALARS[c_type]
    if is_return:
        assert c_type == "char*", f"no ctypes return type for {c_type!r}"          # const char* ac_last_error(void)
        return C.c_char_p
    assert re.fullmatch(r"\w+( \w+)*\*+", c_type), f"no ctypes type for {c_type!r}"
    return C.POINTER(C.c_void_p) if c_type == "ac_ctx**" else C.c_void_p


def defined_version(header: str, version_fn: str) -> int:
    """`#define AC_<X>_ABI_VERSION n` of the header whose version function is ac_<x>_abi_version."""
    found = re.findall(rf"^\s*#define\s+{version_fn.upper()}\s+(\d+)\b", code(header), flags=re.M)
    assert len(found) == 1, f"{header}: {len(found)} definitions of {version_fn.upper()}"
    return int(found[0])
