"""include/audiocut_hip_final.h: the header, the exports and the ctypes signatures agree, the other ABI surfaces are untouched, and
every precondition of ac_tdf_linear_final_f16x3 is refused on the host before anything is launched.  CPU only."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _names(header: str) -> set:
    return set(re.findall(r"\b(ac_[a-z0-9_]+)\s*\(", (ROOT / "include" / header).read_text()))


@pytest.fixture(scope="module")
def lib():
    from audio_cut_amd import _native
    if not _native.library_path().exists():
        subprocess.run(["make", "-C", str(ROOT / "audio_cut_amd" / "csrc")], check=True)
    return _native.load()


def test_final_header_symbols_exported_and_bound(lib):
    from audio_cut_amd import _native
    names = _names("audiocut_hip_final.h")
    assert names == set(_native.FINAL_SIGNATURES) == {"ac_final_abi_version", "ac_tdf_linear_final_f16x3"}
    for name in names:
        assert hasattr(lib, name), f"{name} declared in the final-layer header but not exported"
    assert lib.ac_final_abi_version() == 1
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "audiocut_hip_final.h").read_text(), flags=re.S)
    for name, args in re.findall(r"\bint\s+(ac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(_native.FINAL_SIGNATURES[name][1]), name
    main = _names("audiocut_hip.h")                                    # the other surfaces are untouched
    assert main == set(_native.SIGNATURES) and not (main & names)
    assert lib.ac_abi_version() == 6 and lib.ac_profile_abi_version() == 1
    others = ("stereo", "onset", "beat", "hybrid", "export", "asr", "profile")
    assert not any(names & _names(f"audiocut_hip_{o}.h") for o in others)


def test_final_entry_refuses_every_shape_outside_its_tile(lib):
    """AC_E_INVALID with a message for each precondition; the checks never read the context or the buffers, so placeholders stand
    in for them here (no device on this machine)."""
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    call = lib.ac_tdf_linear_final_f16x3
    ok = dict(ctx=buf, x=buf, wp=buf, sc=buf, sh=buf, resid=buf, fw=buf, fb=buf, spec=buf, y=None, M=48 * 2, N=192, K=32, T=2, C=48, C_out=4)
    cases = [({"ctx": None}, "null pointer"), ({"x": None}, "null pointer"), ({"wp": None}, "null pointer"), ({"spec": None}, "null pointer"),
             ({"resid": None}, "residual"), ({"fw": None}, "final conv"), ({"fb": None}, "final conv"),
             ({"C": 40, "M": 80}, "96 % C"), ({"C": 96, "M": 96, "T": 1}, "C == 48"), ({"C": 16, "M": 96, "T": 6}, "C == 48"),
             ({"T": 3, "M": 144}, "T % (96 / C)"), ({"M": 100}, "items x C x T"), ({"M": 0}, "items x C x T"),
             ({"N": 96}, "N % 192"), ({"N": 0}, "N % 192"), ({"K": 48}, "K % 32"), ({"K": 0}, "K % 32"),
             ({"C_out": 0}, "C_out"), ({"C_out": 5}, "C_out"),
             ({"M": 96 << 40, "N": 192 << 10}, "grid too large")]
    for change, word in cases:
        a = {**ok, **change}
        rc = call(a["ctx"], a["x"], a["wp"], a["sc"], a["sh"], a["resid"], a["fw"], a["fb"], a["spec"], a["y"], a["M"], a["N"], a["K"],
                  a["T"], a["C"], a["C_out"], 1.0, None, None)
        assert rc == -1, change
        msg = lib.ac_last_error().decode()
        assert "invalid argument" in msg and word in msg, (change, msg)


def test_final_tileable_matches_the_entry_conditions():
    from audio_cut_amd._native import Context
    assert Context.tdf_final_tileable(48, 256, 384, 3072, 4) and Context.tdf_final_tileable(48, 2, 32, 192, 1)
    for bad in ((40, 2, 32, 192, 4), (96, 2, 32, 192, 4), (48, 3, 32, 192, 4), (48, 2, 48, 192, 4), (48, 2, 32, 96, 4), (48, 2, 32, 192, 5),
                (48, 2, 32, 192, 0)):
        assert not Context.tdf_final_tileable(*bad), bad
