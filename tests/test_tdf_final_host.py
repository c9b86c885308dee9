"""include/audiocut_hip_final.h: every precondition of ac_tdf_linear_final_f16x3 is refused on the host before anything is
launched, and `Context.tdf_final_tileable` states the same conditions.  CPU only."""
import ctypes as C

from abi_surface import lib  # noqa: F401  (the fixture)


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
