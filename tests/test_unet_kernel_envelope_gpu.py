"""The U-Net MFMA kernels at the edges of what their launchers accept, on inputs whose result is exact by construction
(tests/unet_exact.py): the output must equal the float64 reference BIT FOR BIT - any accumulation, tile or work order - so a dropped,
duplicated or misplaced tap, k-step, lane or low-part term cannot hide in a tolerance.  Shapes are the smallest that reach each path
(the reason each stays in bounds is next to it in unet_exact.CASES); one Gaussian run per shape at the tolerances of
tests/test_unet_gpu.py; and one shape just outside every AC_REQUIRE of the nine launchers, which must be refused by name."""
import numpy as np
import pytest
import torch

import unet_exact as UE
from audio_cut_amd import _native
from audio_cut_amd.separation import conv_pack as CP
from test_unet_gpu import _blk_amax

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in UE.CASES]
TAKES_AMAX = {c[0]: c[3] for c in UE.CASES}
KIND = {c[0]: c[1] for c in UE.CASES}


def _i16(ctx, packed):
    return torch.from_numpy(packed.view(np.int16)).to(ctx.device)


def run_case(ctx, case, in_amax=None, out_amax=None, upload=None, out=None):
    """the kernel of `case` on its tensors (weights packed by conv_pack as the product does).  `upload`: how a host tensor reaches the
    device (default `.to(ctx.device)`); `out`: passed on as `out=` by the 3x3 convs, the wrappers that take one."""
    put = (lambda t: t.to(ctx.device)) if upload is None else (lambda t: upload(t.contiguous().numpy()))
    d = {k: put(v) for k, v in case.t.items()}
    s, kind = case.shapes, case.kind
    ia = None if in_amax is None else put(in_amax)
    _i16 = lambda c, packed: put(torch.from_numpy(packed.view(np.int16)))
    if kind in ("conv", "conv_s8", "conv_w96", "first"):
        w = case.t["w"].numpy()
        packed, un = CP.pack_conv3x3(w) if kind == "conv" else CP.pack_conv3x3_w96(w, 96 if kind == "conv_w96" else 48)
        relu = s.get("relu", True)
        if kind == "first":
            gain, offs = float(case.t["w1"].abs().sum(dim=1).max()), float(case.t["b1"].abs().max())
            return ctx.conv3x3_f16x3_first(d["spec"], d["w1"], d["b1"], _i16(ctx, packed), d["bias"], s["Co"], un, relu=relu, spec_amax=ia,
                                           amax_gain=gain, amax_offs=offs, out_amax=out_amax)
        fn = {"conv": ctx.conv3x3_f16x3, "conv_s8": ctx.conv3x3_f16x3_s8, "conv_w96": ctx.conv3x3_f16x3_w96}[kind]
        return fn(d["x"], _i16(ctx, packed), d["bias"], s["Co"], un, relu=relu, out=out, in_amax=ia, out_amax=out_amax)
    if kind == "tdf":
        packed, un = CP.pack_linear(case.t["w"].numpy())
        return ctx.tdf_linear_f16x3(d["x"], _i16(ctx, packed), s["N"], d["scale"], d["shift"], un, resid=d.get("resid"), in_amax=ia, out_amax=out_amax)
    if kind == "tdf_small":
        p1, p2 = CP.pack_tdf_small(case.t["w1"].numpy(), case.t["w2"].numpy())
        return ctx.tdf_small_fused(d["x"], put(torch.from_numpy(p1)), put(torch.from_numpy(p2)), s["Hd"], d["s1"], d["b1"],
                                   d["s2"], d["b2"], out_amax=out_amax)
    if kind in ("down", "up"):
        packed, un = CP.pack_linear(case.t["wm"].numpy(), bn=96)
        if kind == "down":
            return ctx.down2x_f16x3(d["x"], _i16(ctx, packed), d["bias"], s["Co"], un, in_amax=ia, out_amax=out_amax)
        return ctx.up2x_f16x3(d["x"], _i16(ctx, packed), d["bias"], s["Co"], un, skip=d.get("skip"), in_amax=ia, out_amax=out_amax)
    return ctx.conv1x1_small(d["x"], d["w"], d["bias"], relu=s.get("relu", True))


def _assert_exact(got, case, what):
    diff = (got.double().cpu() - case.ref64).abs()
    print(f"{what}: max |got - ref64| = {float(diff.max()):.3e} over {int((diff != 0).sum())} of {diff.numel()} elements")
    assert torch.equal(got.double().cpu(), case.ref64), what


@pytest.mark.parametrize("case_id", IDS)
def test_exact_on_both_grids(hip_ctx, case_id):
    """Bit-identical to float64 on the x-lo and the w-lo grid (the true-float32 kernels: both operands on the grid); where the
    kernel takes amax: unchanged by asking for out_amax, which is the exact per-row maximum, and still exact with in_amax = the true
    row maxima of rows at different power-of-two levels (the common-scale path; up2x: a wave straddling two rows has two scales)."""
    kind = KIND[case_id]
    for grid in UE.grids_of(kind):
        case = UE.case_of(case_id, grid)
        y = run_case(hip_ctx, case)
        _assert_exact(y, case, f"{case_id}/{grid}")
        if not TAKES_AMAX[case_id]:
            continue
        oa = torch.zeros((y.shape[0], y.shape[2]), device=hip_ctx.device)
        assert torch.equal(run_case(hip_ctx, case, out_amax=oa), y), f"{case_id}/{grid}: out_amax changes the result"
        assert torch.equal(oa, _blk_amax(y)), f"{case_id}/{grid}: out_amax"
        if kind in UE.SPLIT_KINDS:
            lv = UE.case_of(case_id, grid, levels=True)
            oa.zero_()
            y = run_case(hip_ctx, lv, in_amax=lv.in_amax, out_amax=oa)
            _assert_exact(y, lv, f"{case_id}/{grid}/in_amax")
            assert torch.equal(oa, _blk_amax(y)), f"{case_id}/{grid}/in_amax: out_amax"


@pytest.mark.parametrize("case_id", IDS)
def test_gaussian_at_the_existing_tolerance(hip_ctx, case_id):
    """Gaussian inputs against float64 at the tolerance tests/test_unet_gpu.py holds that kernel to (relative to the peak)."""
    case = UE.case_of(case_id, "gauss")
    y = run_case(hip_ctx, case).double().cpu()
    err = float((y - case.ref64).abs().max() / case.ref64.abs().max())
    print(f"{case_id}: {err:.2e}")
    assert y.shape == case.ref64.shape and err < UE.GAUSS_TOL[case.kind], (case_id, err)


@pytest.mark.parametrize("case_id", [i for i in IDS if KIND[i] == "first"])
def test_first_is_bit_identical_to_conv1x1_then_s8(hip_ctx, case_id):
    """ac_conv3x3_f16x3_first == ac_conv1x1_small followed by ac_conv3x3_f16x3_s8, bit for bit, for C0 in {1, 3, 4}, C_in in
    {16, 48, 64}, one tile and 16 x 64."""
    dev = hip_ctx.device
    for grid in ("xlo", "gauss"):
        case = UE.case_of(case_id, grid)
        t = case.t
        packed, un = CP.pack_conv3x3_w96(t["w"].numpy(), 48)
        mid = hip_ctx.conv1x1_small(t["spec"].to(dev), t["w1"].to(dev), t["b1"].to(dev), relu=True)
        ref = hip_ctx.conv3x3_f16x3_s8(mid, _i16(hip_ctx, packed), t["bias"].to(dev), 48, un, relu=True)
        assert torch.equal(run_case(hip_ctx, case), ref), (case_id, grid)


# ---- refusals: one shape just outside each AC_REQUIRE; nothing is launched ----------------------------------------------------
def _z(ctx, *shape):
    return torch.zeros(*shape, device=ctx.device)


def _wp(ctx, n_bytes):
    return torch.zeros(max(int(n_bytes or 4), 4) // 2, dtype=torch.int16, device=ctx.device)


def _conv_call(fn_name, cob, stage, B=1, Ci=16, Co=None, H=8, W=32, bias=True):
    def call(ctx):
        co = cob if Co is None else Co
        out = torch.full((B, co, H, W), 7.0, device=ctx.device)
        try:
            getattr(ctx, fn_name)(_z(ctx, B, Ci, H, W), _wp(ctx, _native._conv3x3_packed_bytes(Ci, co, cob, stage)),
                                  _z(ctx, co) if bias else None, co, 1.0, out=out)
        finally:
            assert bool((out == 7.0).all()), "a refused call wrote to out="
    return call


def _first_call(C0=4, Ci=16, gain=1.0, b1=True):
    return lambda ctx: ctx.conv3x3_f16x3_first(_z(ctx, 1, C0, 8, 32), _z(ctx, Ci, C0), _z(ctx, Ci) if b1 else None,
                                               _wp(ctx, _native._conv3x3_packed_bytes(Ci, 48, 48, 8)), _z(ctx, 48), 48, 1.0, amax_gain=gain)


def _tdf_call(C=16, T=8, K=32, N=96, scale=True):
    return lambda ctx: ctx.tdf_linear_f16x3(_z(ctx, 1, C, T, K), _wp(ctx, _native._linear_packed_bytes(N, K, 0)), N,
                                            _z(ctx, C) if scale else None, _z(ctx, C), 1.0)


def _small_call(B=1, C=4, T=8, Fq=32, Hd=12, amax=False, s1=True):
    def call(ctx):
        p1, p2 = CP.pack_tdf_small(np.ones((12, 32), np.float32), np.ones((32, 12), np.float32))
        if Fq % 32 == 0 and 0 < Hd <= 48:
            p1, p2 = CP.pack_tdf_small(np.ones((Hd, Fq), np.float32), np.ones((Fq, Hd), np.float32))
        ctx.tdf_small_fused(_z(ctx, B, C, T, Fq), torch.from_numpy(p1).to(ctx.device), torch.from_numpy(p2).to(ctx.device), Hd,
                            _z(ctx, C) if s1 else None, _z(ctx, C), _z(ctx, C), _z(ctx, C), out_amax=_z(ctx, B, T) if amax else None)
    return call


def _rs_call(mode, Ci=8, Co=24, H=16, W=32, amax=False, bias=True):
    def call(ctx):
        x = _z(ctx, 1, Ci, H, W)
        ia = _z(ctx, 1, H) if amax else None
        b = _z(ctx, Co) if bias else None
        if mode == "down":
            ctx.down2x_f16x3(x, _wp(ctx, _native._linear_packed_bytes(Co, 4 * Ci, 96)), b, Co, 1.0, in_amax=ia)
        else:
            ctx.up2x_f16x3(x, _wp(ctx, _native._linear_packed_bytes(4 * Co, Ci, 96)), b, Co, 1.0, in_amax=ia)
    return call


def _c11_call(B=1, Ci=4, Co=8, P=4, bias=True):
    return lambda ctx: ctx.conv1x1_small(_z(ctx, B, Ci, 1, P), _z(ctx, Co, Ci), _z(ctx, Co) if bias else None, relu=True)


def _raw(name, *args):
    """the C entry point itself, for the conditions no wrapper call can reach (sizes whose tensors cannot exist, x == y): every
    pointer is one small live buffer, which a refused call never touches; `args` follow the context handle, None = that buffer,
    "Q" = its second half (an output distinct from the input).
    These calls are safe ONLY because the AC_REQUIRE each one targets comes before the launch (read in csrc/: every AC_REQUIRE of a
    launcher precedes its hipLaunchKernelGGL, and the size tests are made in 64-bit arithmetic): with such sizes no launch could stay
    inside any buffer.  Whoever removes or reorders one of those conditions must remove its case here first."""
    def call(ctx):
        buf = _z(ctx, 1024)
        rc = getattr(ctx.lib, name)(ctx._h, *[buf.data_ptr() if a is None else (buf.data_ptr() + 2048 if a == "Q" else a) for a in args], _native._stream())
        assert bool((buf == 0).all())
        _native._check(rc)
    return call


_P = None           # a pointer argument of _raw
_REFUSALS = []
for _name, _cob, _st in (("conv3x3_f16x3", 48, 16), ("conv3x3_f16x3_s8", 48, 8), ("conv3x3_f16x3_w96", 96, 8)):
    _REFUSALS += [
        (f"{_name}-C_in24", _conv_call(_name, _cob, _st, Ci=24), "C_in % 16 == 0"),
        (f"{_name}-C_out40", _conv_call(_name, _cob, _st, Co=40), "C_out % 48 == 0" if _name == "conv3x3_f16x3" else "C_out % (96 or 48) == 0"),
        (f"{_name}-H4", _conv_call(_name, _cob, _st, H=4), "H % 8 == 0 and W % 32 == 0"),
        (f"{_name}-W16", _conv_call(_name, _cob, _st, W=16), "H % 8 == 0 and W % 32 == 0"),
        (f"{_name}-null_bias", _conv_call(_name, _cob, _st, bias=False), "null pointer"),
        # H * W = 2^31; B (C_out / cob) (H / 8) (W / 32) = 2^20 * 2^10 * 2^10 workgroups
        (f"{_name}-plane", _raw("ac_" + _name, _P, _P, _P, _P, 1, 16, _cob, 65536, 32768, 1.0, 1, 0, 0), "plane too large"),
        (f"{_name}-grid", _raw("ac_" + _name, _P, _P, _P, _P, 1 << 20, 16, _cob, 8192, 32768, 1.0, 1, 0, 0), "grid too large"),
    ]
_REFUSALS += [
    ("first-C0_5", _first_call(C0=5), "fused first conv"),
    ("first-C_in80", _first_call(Ci=80), "fused first conv"),
    ("first-negative_gain", _first_call(gain=-1.0), "amax bound terms must be non-negative"),
    ("first-null_b1", _first_call(b1=False), "null pointer"),
    ("tdf-C8", _tdf_call(C=8), "C % 16 == 0 and T % 8 == 0"),
    ("tdf-T4", _tdf_call(T=4), "C % 16 == 0 and T % 8 == 0"),
    ("tdf-K48", _tdf_call(K=48), "K % 32 == 0"),
    ("tdf-N48", _tdf_call(N=48), "N % 96 == 0"),
    ("tdf-null_scale", _tdf_call(scale=False), "null pointer"),
    ("tdf-grid", _raw("ac_tdf_linear_f16x3", _P, _P, _P, _P, 0, _P, 1 << 40, 96, 32, 8, 16, 1.0, 0, 0), "grid too large"),
    ("tdf_small-Hd0", _small_call(Hd=0), "bottleneck width in [1, 48]"),
    ("tdf_small-Hd49", _small_call(Hd=49), "bottleneck width in [1, 48]"),
    ("tdf_small-F48", _small_call(Fq=48), "F % 32 == 0"),
    ("tdf_small-M48", _small_call(C=6), "M % 32 == 0"),
    ("tdf_small-amax_CT48", _small_call(B=2, C=3, T=16, amax=True), "amax needs (C * T) % 32 == 0"),
    ("tdf_small-null_scale1", _small_call(s1=False), "null pointer"),
    ("tdf_small-x_is_y", lambda ctx: _small_in_place(ctx), "in-place not supported"),
    ("tdf_small-T0", _raw("ac_tdf_small_fused", _P, _P, _P, _P, _P, _P, _P, "Q", 32, 32, 12, 0, 4, 0), "T, C > 0"),
    ("tdf_small-grid", _raw("ac_tdf_small_fused", _P, _P, _P, _P, _P, _P, _P, "Q", 1 << 38, 32, 12, 8, 4, 0), "grid too large"),
    ("down-H15", _rs_call("down", H=15), "down: H even, W % 4 == 0, C_in % 8 == 0"),
    ("down-W6", _rs_call("down", W=6), "down: H even, W % 4 == 0, C_in % 8 == 0"),
    ("down-C_in4", _rs_call("down", Ci=4), "down: H even, W % 4 == 0, C_in % 8 == 0"),
    ("down-P64", _rs_call("down", H=16, W=16), "pixels per image % 128 == 0"),
    ("down-amax_W12", _rs_call("down", H=128, W=12, amax=True), "down with amax"),
    ("down-null_bias", _rs_call("down", bias=False), "null pointer"),
    ("down-B0", _raw("ac_down2x_f16x3", _P, _P, _P, _P, 0, 8, 24, 16, 32, 1.0, 0, 0), "positive sizes"),
    ("up-C_out20", _rs_call("up", Co=20, H=4), "up: W % 4 == 0, 4 * C_out % 96 == 0"),
    ("up-W6", _rs_call("up", H=64, W=6), "up: W % 4 == 0, 4 * C_out % 96 == 0"),
    ("up-P64", _rs_call("up", H=2, W=32), "pixels per image % 128 == 0"),
    ("up-amax_W32", _rs_call("up", H=4, W=32, amax=True), "up with amax"),
    # H * W * 4 = 2^31; B (H W / 128) = 2^20 * 2^13 workgroups
    ("up-plane", _raw("ac_up2x_f16x3", _P, _P, _P, 0, _P, 1, 8, 24, 32768, 16384, 1.0, 0, 0), "plane too large"),
    ("up-grid", _raw("ac_up2x_f16x3", _P, _P, _P, 0, _P, 1 << 20, 8, 24, 1024, 1024, 1.0, 0, 0), "grid too large"),
    ("conv1x1-9to9", _c11_call(Ci=9, Co=9), "one of C_in, C_out must be <= 8"),
    ("conv1x1-P6", _c11_call(P=6), "B <= 65535, P % 4 == 0"),
    ("conv1x1-B65536", _c11_call(B=65536), "B <= 65535, P % 4 == 0"),
    ("conv1x1-null_bias", _c11_call(bias=False), "null pointer"),
]


def _small_in_place(ctx):
    x = _z(ctx, 1, 4, 8, 32)
    p1, p2 = CP.pack_tdf_small(np.ones((12, 32), np.float32), np.ones((32, 12), np.float32))
    v = _z(ctx, 4)
    rc = ctx.lib.ac_tdf_small_fused(ctx._h, x.data_ptr(), torch.from_numpy(p1).to(ctx.device).data_ptr(), torch.from_numpy(p2).to(ctx.device).data_ptr(),
                                    v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), x.data_ptr(), 32, 32, 12, 8, 4, None, _native._stream())
    _native._check(rc)


@pytest.mark.parametrize("rid", [r[0] for r in _REFUSALS])
def test_shapes_outside_the_envelope_are_refused_by_name(hip_ctx, rid):
    """NativeError (not a bare Exception), ac_last_error names the violated condition, an `out=` buffer keeps its sentinel."""
    _, call, needle = _REFUSALS[[r[0] for r in _REFUSALS].index(rid)]
    with pytest.raises(_native.NativeError) as info:
        call(hip_ctx)
    assert "invalid argument" in str(info.value) and needle in str(info.value), str(info.value)
    assert needle in hip_ctx.lib.ac_last_error().decode()
