"""ac_tdf_linear_final_f16x3 (the last TDF layer with the graph's final 1x1 conv in its epilogue) against the two kernels it replaces,
run one after the other: conv1x1_small(tdf_linear_f16x3(h, ..., resid=x, in_amax=ah), final_w, final_b, relu=False).  Equality of
bits, on the spectrogram and on the optional y; no tolerance anywhere.

The unfused TDF kernel tiles 8 time rows, the fused one 2, so T = 2 and T = 6 exist for the fused kernel only.  Their reference
is the same pair of kernels on the case padded to 8 time rows (zero rows of h, of the residual and of the maxima behind the real
ones), cut back to T: a GEMM row sees only its own row of h, its own time row's maximum, its channel and its residual, and the 1x1
conv works per pixel, so the padded run computes the T real rows exactly as an 8-row-tiled T would."""
import ctypes as C

import numpy as np
import pytest
import torch

from audio_cut_amd import _native
from audio_cut_amd.separation.conv_pack import pack_linear

pytestmark = pytest.mark.gpu


def _case(dev, b, c, t, k, n, c_out, seed, zero_row=None, spread=False):
    """Seeded inputs as in test_tdf_linear_f16x3_kernel (asymmetric weights: a transposed operand shows); `zero_row`: that time row
    of h is all zero (amax 0: the no-scale path) with its residual left non-zero; `spread`: odd time rows 2^-20 of the even ones,
    so the two rows of every 2-row tile need scales 2^20 apart."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(b, c, t, k, generator=g) * 3
    if spread:
        h[:, :, 1::2, :] *= 2.0 ** -20
    if zero_row is not None:
        h[:, :, zero_row, :] = 0.0
    wt = torch.randn(n, k, generator=g) / np.sqrt(k)
    sc = torch.rand(c, generator=g) + 0.5
    sh = torch.randn(c, generator=g) * 0.3
    resid = torch.randn(b, c, t, n, generator=g)
    fw = torch.randn(c_out, c, generator=g) / np.sqrt(c)
    fb = torch.randn(c_out, generator=g) * 0.1
    packed, unscale = pack_linear(wt.numpy())
    d = dict(h=h, sc=sc, sh=sh, resid=resid, fw=fw, fb=fb, wp=torch.from_numpy(packed.view(np.int16)))
    d = {name: v.to(dev).contiguous() for name, v in d.items()}
    d["amax"] = d["h"].abs().amax(dim=(1, 3)).contiguous()             # [B, T]: the true maximum of every time row
    d["unscale"], d["n"] = unscale, n
    return d


def _unfused(ctx, d):
    """The yardstick: the two existing kernels one after the other (on 8-row-padded operands where T % 8 != 0, see the module text)."""
    h, resid, amax = d["h"], d["resid"], d["amax"]
    b, c, t, k = h.shape
    tp = -(-t // 8) * 8
    if tp != t:
        pad = lambda x, shape: torch.cat([x, torch.zeros(shape, device=x.device)], dim=2 if x.dim() == 4 else 1).contiguous()
        h, resid, amax = pad(h, (b, c, tp - t, k)), pad(resid, (b, c, tp - t, d["n"])), pad(amax, (b, tp - t))
    y = ctx.tdf_linear_f16x3(h, d["wp"], d["n"], d["sc"], d["sh"], d["unscale"], resid=resid, in_amax=amax)
    spec = ctx.conv1x1_small(y, d["fw"], d["fb"], relu=False)
    return spec[:, :, :t].contiguous(), y[:, :, :t].contiguous()


def _fused(ctx, d, want_y):
    return ctx.tdf_linear_final_f16x3(d["h"], d["wp"], d["n"], d["sc"], d["sh"], d["unscale"], d["resid"], d["fw"], d["fb"],
                                      in_amax=d["amax"], want_y=want_y)


# (B, C, T, K, N), C_out, extras
CASES = {
    "one_workgroup_one_stage": ((1, 48, 2, 32, 192), 4, {}),                               # one column block
    "items_tiles_both_buffers": ((2, 48, 8, 64, 384), 4, {"spread": True}),              # item stride, four row tiles, two column blocks
    "t6_odd_stage_count": ((1, 48, 6, 96, 192), 4, {"zero_row": 3}),                     # T % 8 != 0, three stages, an all-zero time row
    "three_output_channels": ((2, 48, 8, 64, 384), 3, {}),
    "one_output_channel": ((1, 48, 2, 32, 192), 1, {"zero_row": 0}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_final_is_the_two_kernels_bit_for_bit(hip_ctx, name):
    shape, c_out, extra = CASES[name]
    d = _case(hip_ctx.device, *shape, c_out, seed=11 + len(name), **extra)
    ref_spec, ref_y = _unfused(hip_ctx, d)
    if extra.get("zero_row") is not None:
        z = extra["zero_row"]
        assert float(d["amax"][:, z].max()) == 0.0 and float(d["resid"][:, :, z].abs().min()) > 0.0
        assert torch.equal(ref_y[:, :, z], d["resid"][:, :, z] + torch.relu(d["sh"]).view(1, -1, 1))      # the row is its shift and residual alone
    if extra.get("spread"):
        ratio = d["amax"][:, 0::2] / d["amax"][:, 1::2]
        assert float(ratio.min()) > 2.0 ** 19 and float(ratio.max()) < 2.0 ** 21
    spec, y = _fused(hip_ctx, d, want_y=True)
    assert spec.shape == ref_spec.shape == (shape[0], c_out, shape[2], shape[4])
    assert torch.equal(y, ref_y), f"y differs in {int((y != ref_y).sum())} of {y.numel()} values"
    assert torch.equal(spec, ref_spec), f"spectrogram differs in {int((spec != ref_spec).sum())} of {spec.numel()} values"
    only = _fused(hip_ctx, d, want_y=False)                                                # y == NULL: the product's call
    assert torch.equal(only, ref_spec)
    assert float(ref_spec.abs().max()) > 0.1 and bool(torch.isfinite(ref_spec).all())      # a comparison of real values


def test_shapes_outside_the_tile_are_refused_and_nothing_is_written(hip_ctx):
    dev = hip_ctx.device
    d = _case(dev, 1, 48, 2, 32, 192, 4, seed=5)
    for what, (c, t, n) in {"C = 40": (40, 2, 192), "T = 3": (48, 3, 192), "N = 96": (48, 2, 96)}.items():
        z = lambda *s: torch.zeros(*s, device=dev)
        wp = torch.zeros(2 * n * 32, dtype=torch.int16, device=dev)
        with pytest.raises(_native.NativeError, match="invalid argument"):
            hip_ctx.tdf_linear_final_f16x3(z(1, c, t, 32), wp, n, z(c), z(c), 1.0, z(1, c, t, n), z(4, c), z(4), want_y=True)
        # the library itself, with outputs it could have written into: refused before any launch, every value still the sentinel
        spec = torch.full((1, 4, t, n), 7.0, device=dev)
        y = torch.full((1, c, t, n), 7.0, device=dev)
        x, r, w4, s = z(1, c, t, 32), z(1, c, t, n), z(4, c), z(c)
        p = lambda v: C.c_void_p(v.data_ptr())
        rc = hip_ctx.lib.ac_tdf_linear_final_f16x3(hip_ctx._h, p(x), p(wp), p(s), p(s), p(r), p(w4), p(s), p(spec), p(y), c * t, n, 32, t, c, 4,
                                                   1.0, None, None)
        torch.cuda.synchronize()
        assert rc == -1 and b"invalid argument" in hip_ctx.lib.ac_last_error(), what
        assert bool((spec == 7.0).all()) and bool((y == 7.0).all()), what
    # K % 32, C_out outside 1..4, a missing residual or final weight: refused likewise
    p = lambda v: C.c_void_p(v.data_ptr())
    spec = torch.full((1, 4, 2, 192), 7.0, device=dev)
    base = dict(x=p(d["h"]), wp=p(d["wp"]), sc=p(d["sc"]), sh=p(d["sh"]), resid=p(d["resid"]), fw=p(d["fw"]), fb=p(d["fb"]), K=32, C_out=4)
    for change in ({"K": 48}, {"C_out": 0}, {"C_out": 5}, {"resid": None}, {"fw": None}, {"fb": None}):
        a = {**base, **change}
        rc = hip_ctx.lib.ac_tdf_linear_final_f16x3(hip_ctx._h, a["x"], a["wp"], a["sc"], a["sh"], a["resid"], a["fw"], a["fb"], p(spec), None,
                                                   48 * 2, 192, a["K"], 2, 48, a["C_out"], 1.0, None, None)
        assert rc == -1, change
    torch.cuda.synchronize()
    assert bool((spec == 7.0).all())
    # the wrapper's own checks: packed weights of another size, a residual of another shape
    with pytest.raises(_native.NativeError, match="bytes, the shape implies"):
        hip_ctx.tdf_linear_final_f16x3(d["h"], d["wp"][:-1], 192, d["sc"], d["sh"], 1.0, d["resid"], d["fw"], d["fb"])
    with pytest.raises(_native.NativeError, match="residual"):
        hip_ctx.tdf_linear_final_f16x3(d["h"], d["wp"], 192, d["sc"], d["sh"], 1.0, d["resid"][:, :, :1], d["fw"], d["fb"])


def test_whole_net_takes_the_fused_path_and_matches_the_tapped_one(hip_ctx):
    """One full [1, 4, 256, 3072] item, seeded weights: forward_tf without a block tap (fused last launch) == with one (the two kernels)."""
    from audio_cut_amd.separation.tfc_tdf import TfcTdfNet, TfcTdfSpec, synth_weights
    spec = TfcTdfSpec()
    net = TfcTdfNet(synth_weights(spec, seed=0), spec, hip=hip_ctx).to(hip_ctx.device).eval()
    x = (torch.randn(1, 4, 256, 3072, generator=torch.Generator().manual_seed(2)) * 0.5).to(hip_ctx.device)
    calls = {"fused": 0, "conv1x1": 0}
    fused, conv = hip_ctx.tdf_linear_final_f16x3, hip_ctx.conv1x1_small
    hip_ctx.tdf_linear_final_f16x3 = lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), fused(*a, **k))[1]
    hip_ctx.conv1x1_small = lambda *a, **k: (calls.__setitem__("conv1x1", calls["conv1x1"] + 1), conv(*a, **k))[1]
    try:
        y_fused = net.forward_tf(x)
        assert calls == {"fused": 1, "conv1x1": 0}
        taps = []
        net.block_tap = lambda name, t: taps.append(name)
        y_tapped = net.forward_tf(x)
        assert calls == {"fused": 1, "conv1x1": 1} and taps[-1] == f"dec{spec.n_levels - 1}"
    finally:
        net.block_tap = None
        del hip_ctx.tdf_linear_final_f16x3, hip_ctx.conv1x1_small
    assert y_fused.shape == y_tapped.shape == x.shape
    assert torch.equal(y_fused, y_tapped)
    assert float(y_fused.abs().max()) > 0.0 and bool(torch.isfinite(y_fused).all())
