"""Inputs for the U-Net MFMA kernels whose result is EXACT by construction, and a numpy emulation of the split-f16 GEMM.

The split-float16 kernels compute xh*wh + xh*wl + xl*wh (float16 pairs, float32 accumulation) and drop xl*wl.  A case built here
makes every one of those products, every partial sum in ANY order and every epilogue step an exactly representable float32, so a
kernel's output must equal the float64 reference bit for bit whatever its tiling, accumulation order or work order - a dropped,
duplicated or misplaced tap, k-step, lane or low-part term changes an integer multiple of the grid step and cannot hide in rounding.

Grids ("x" = activations, "w" = weights):
  xlo   x = a + b * 2^-10 (a in -3..3, b in -3..3: about a third of the values need the float16 low part), w / bias / shift small
        integers, TDF scales small integers or powers of two: pins the xl*wh term
  wlo   the roles swapped (conv_pack.weight_scale is a power of two, so packing stays exact): pins the xh*wl term
  both  both operands on the grid (a in -1..1): the true-float32 kernels only
  gauss Gaussian inputs as in tests/test_unet_gpu.py: no exactness claim, compared at that file's tolerances
`make_case` ASSERTS, in numpy / torch on the CPU, the conditions under which the claim holds (`_check_split`, `_check_sums`), so a
case that is not exact never reaches a GPU assertion:
  split     at the power-of-two scale the kernel uses (1 without in_amax; with it the scale of ac_row_ex / ac_act_scale_lane in
            csrc/ac_common.h over the rows that kernel takes the maximum of) x*s == f16(x*s) + f16(x*s - f16(x*s)) with the low part
            zero or a NORMAL float16, nothing clamps at 65504, and one of the two operands has no low part at all (xl*wl == 0)
  sums      for every output element sum |x||w| + |bias| (times |scale|) < 2^24 * lsb, lsb = the grid step of the products: every
            partial sum is a multiple of lsb below 2^24 lsb, i.e. a float32; for the two-stage kernels (tdf_small_fused,
            conv3x3_f16x3_first) the same on the first stage's actual output
  result    the float64 reference is a float32
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from audio_cut_amd.separation import conv_pack as CP

GRID = 2.0 ** -10
ROWX_SPREAD = 12            # AC_ROWX_SPREAD (csrc/ac_common.h): a conv tile whose row maxima span more takes the row-exact path
SPLIT_KINDS = ("conv", "conv_s8", "conv_w96", "first", "tdf", "down", "up")
F32_KINDS = ("tdf_small", "conv1x1")
# tolerances of tests/test_unet_gpu.py (error relative to the reference's peak), per kernel; `first`: the kernel behind it (_s8)
GAUSS_TOL = {"conv": 2e-6, "conv_s8": 2e-6, "conv_w96": 2e-6, "first": 2e-6, "tdf": 3e-6, "down": 2e-6, "up": 2e-6,
             "tdf_small": 1e-6, "conv1x1": 1e-6}


@dataclass
class Case:
    kind: str
    shapes: dict
    grid: str
    t: Dict[str, torch.Tensor]                     # float32 CPU tensors, named as the wrapper's arguments
    ref64: torch.Tensor
    in_amax: Optional[torch.Tensor] = None         # [B, H] float32: the true per-row maximum of the input (levels=True)
    # GEMM view of the (last) split stage for `emulate`: A [M, K], row scale s [M], W [N, K], weight scale, epilogue, one tap's columns
    gemm: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' activation scale (csrc/ac_common.h)
def row_ex_scale(a: np.ndarray) -> np.ndarray:
    """power of two that puts a in [2^14, 2^15) (ac_row_ex / ac_act_scale_lane); 1 where a is not a usable maximum."""
    a = np.asarray(a, np.float32)
    _, e = np.frexp(a)                              # a = m * 2^e, m in [0.5, 1)
    ex = np.clip(15 - e, -120, 120)
    ok = (a > 0) & (a < 3.0e38)
    return np.where(ok, np.ldexp(np.float32(1), ex), np.float32(1)).astype(np.float32)


def kernel_row_scale(kind: str, amax: Optional[np.ndarray], b: int, h_in: int, gain: float = 1.0, offs: float = 0.0) -> np.ndarray:
    """[B, H_out rows of the GEMM's M axis] scale the kernel applies to the activations that enter output row y of item b."""
    if kind == "down":
        h_out = h_in // 2
    else:
        h_out = h_in
    if amax is None:
        return np.ones((b, h_out), np.float32)
    a = (np.asarray(amax, np.float32) * np.float32(gain) + np.float32(offs)).astype(np.float32)
    if kind in ("tdf", "up"):                       # a GEMM row's own time row / an up-sampling pixel's own input row
        return row_ex_scale(a)
    if kind == "down":                              # the two input rows of an output pixel
        return row_ex_scale(np.maximum(a[:, 0::2], a[:, 1::2]))
    out = np.ones((b, h_in), np.float32)            # 3x3 convs: the ten patch rows y0 - 1 .. y0 + 8 of the 8-row tile
    for y0 in range(0, h_in, 8):
        rows = a[:, max(0, y0 - 1):min(h_in, y0 + 9)]
        live = np.where(rows > 0, rows, np.nan)
        with np.errstate(all="ignore"):
            spread = np.log2(np.nanmax(live, axis=1) / np.nanmin(live, axis=1))
        assert not (np.nan_to_num(spread) > ROWX_SPREAD).any(), "tile would take the row-exact path"
        out[:, y0:y0 + 8] = row_ex_scale(rows.max(axis=1))[:, None]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the conditions of exactness
def split16(v: np.ndarray):
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def _lsb(*arrays) -> float:
    """largest power of two every value of the arrays is a multiple of."""
    p = 2.0 ** 8
    vals = np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays])
    while p > 2.0 ** -60:
        q = vals / p
        if np.array_equal(q, np.round(q)):
            return p
        p /= 2
    raise AssertionError("values are not on a power-of-two grid")


def _check_split(name: str, v: np.ndarray, scale) -> np.ndarray:
    """v * scale (a power of two per element) splits exactly into float16 hi + lo with a zero or normal low part; -> lo."""
    vs = (np.asarray(v, np.float32) * np.asarray(scale, np.float32)).astype(np.float32)
    assert np.array_equal(vs.astype(np.float64), np.asarray(v, np.float64) * np.asarray(scale, np.float64)), f"{name}: scaling is not exact"
    assert float(np.abs(vs).max(initial=0.0)) <= 65504.0, f"{name}: clamps at the float16 range"
    hi, lo = split16(vs)
    assert np.array_equal(hi + lo, vs), f"{name}: hi + lo != value"
    assert np.all((lo == 0) | (np.abs(lo) >= 2.0 ** -14)), f"{name}: subnormal low part"
    return lo


def _check_sums(name: str, abs_sum: torch.Tensor, lsb: float) -> None:
    """every partial sum of the accumulation is a float32: sum |x||w| + |b| (the split's parts add at most 2^-9 of it) < 2^24 lsb."""
    worst = float(abs_sum.max()) * (1.0 + 2.0 ** -9)
    assert worst < 2.0 ** 24 * lsb, f"{name}: partial sums reach {worst:.1f} >= 2^24 * {lsb}"


def _check_f32(name: str, t: torch.Tensor) -> None:
    assert torch.equal(t.float().double(), t), f"{name}: the float64 reference is not a float32"


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
def _grid(rng, shape, lo_part: bool, a_max: int = 3, density: float = 1.0) -> torch.Tensor:
    a = rng.integers(-a_max, a_max + 1, size=shape).astype(np.float64)
    if lo_part:
        a = a + rng.integers(-3, 4, size=shape) * GRID
    if density < 1.0:
        a = a * (rng.random(size=shape) < density)
    return torch.from_numpy(a.astype(np.float32))


def _ints(rng, shape, m: int) -> torch.Tensor:
    return torch.from_numpy(rng.integers(-m, m + 1, size=shape).astype(np.float32))


def _apply_levels(rng, x: torch.Tensor) -> torch.Tensor:
    """rows of the time axis (dim 2) at different power-of-two levels 1, 2, 4 (neighbours differ; well within AC_ROWX_SPREAD)."""
    h = x.shape[2]
    k = (np.arange(h) + np.arange(h) // 5 + rng.integers(0, 3)) % 3      # steps of 1 or 2 (mod 3): neighbouring rows always differ
    lv = torch.from_numpy((2.0 ** k).astype(np.float32)).view(1, 1, h, 1)
    lv = lv.expand(x.shape[0], 1, h, 1).clone()
    if x.shape[0] > 1:
        lv[1] = lv[1].flip(1)                                   # items differ too
    return x * lv


def _blk_amax(t: torch.Tensor) -> torch.Tensor:
    return t.abs().amax(dim=(1, 3)).contiguous()


def _v(a: torch.Tensor) -> torch.Tensor:
    return a.double().view(1, -1, 1, 1)


def make_case(kind: str, shapes: dict, seed: int, grid: str = "xlo", levels: bool = False) -> Case:
    """The tensors of one kernel call and its float64 reference.  grid: "xlo" / "wlo" / "both" (exact; asserted here) or "gauss".
    levels: give the rows of the time axis different power-of-two levels and return the true per-row maximum as `in_amax`."""
    assert kind in SPLIT_KINDS + F32_KINDS and grid in ("xlo", "wlo", "both", "gauss")
    assert grid != "both" or kind in F32_KINDS
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    s = dict(shapes)
    exact = grid != "gauss"
    xl, wl = grid in ("xlo", "both"), grid in ("wlo", "both")
    am = 1 if grid == "both" else 3
    name = f"{kind}{shapes}/{grid}"

    def act(shape, scale=2.0):
        x = _grid(rng, shape, xl, am) if exact else torch.randn(*shape, generator=g) * scale
        return _apply_levels(rng, x) if levels else x

    def wgt(shape, fan_in, density=1.0):
        return _grid(rng, shape, wl, am if grid == "both" else (3 if wl else 2), density) if exact else torch.randn(*shape, generator=g) / np.sqrt(fan_in)

    def vec(n, m=3, std=0.2):
        return _ints(rng, (n,), m) if exact else torch.randn(n, generator=g) * std

    def tdf_scale(n):
        if exact:
            return torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 4.0], np.float32), size=n))
        return torch.rand(n, generator=g) + 0.5

    t: Dict[str, torch.Tensor] = {}
    gemm: dict = {}
    in_amax = None
    if kind in ("conv", "conv_s8", "conv_w96", "first"):
        B, Ci, Co, H, W, relu = s["B"], s["Ci"], s["Co"], s["H"], s["W"], s.get("relu", True)
        gain, offs = 1.0, 0.0
        if kind == "first":
            C0 = s["C0"]
            spec = act((B, C0, H, W), 3.0)
            w1 = _ints(rng, (Ci, C0), 2) if exact else torch.randn(Ci, C0, generator=g) * 0.5
            b1 = vec(Ci, 3, 0.3)
            t.update(spec=spec, w1=w1, b1=b1)
            mid64 = F.relu(F.conv2d(spec.double(), w1.double().view(Ci, C0, 1, 1), b1.double()))
            x32 = F.relu(F.conv2d(spec, w1.view(Ci, C0, 1, 1), b1))            # float32: exact on the grids
            gain, offs = float(w1.abs().sum(dim=1).max()), float(b1.abs().max())
            if exact:
                abs1 = F.conv2d(spec.abs().double(), w1.abs().double().view(Ci, C0, 1, 1), b1.abs().double())
                _check_sums(name + " stage 1", abs1, _lsb(spec, b1) * _lsb(w1))
                assert torch.equal(x32.double(), mid64)
            amax_src = spec
        else:
            x32 = act((B, Ci, H, W))
            t["x"] = x32
            mid64 = x32.double()
            amax_src = x32
        w = wgt((Co, Ci, 3, 3), 9 * Ci)
        bias = vec(Co, 3, 0.1)
        t.update(w=w, bias=bias)
        ref = F.conv2d(mid64, w.double(), bias.double(), padding=1)
        ref = F.relu(ref) if relu else ref
        if levels:
            in_amax = _blk_amax(amax_src)
        rs = kernel_row_scale("conv", None if in_amax is None else in_amax.numpy(), B, H, gain, offs)       # [B, H]
        if exact:
            lo_x = _check_split(name + " x", x32.numpy(), rs[:, None, :, None])
            ws = CP.weight_scale(w.numpy())
            lo_w = _check_split(name + " w", w.numpy(), ws)
            assert not lo_x.any() or not lo_w.any(), f"{name}: xl*wl is not zero"
            _check_sums(name, F.conv2d(mid64.abs(), w.abs().double(), bias.abs().double(), padding=1), _lsb(x32, bias) * _lsb(w))
        A = F.unfold(x32, 3, padding=1).transpose(1, 2).reshape(B * H * W, Ci * 9).numpy()
        bnp = bias.numpy()

        def epi(acc, relu=relu):
            v = acc + bnp[None, :]
            v = np.maximum(v, 0) if relu else v
            return torch.from_numpy(np.ascontiguousarray(v.reshape(B, H, W, Co).transpose(0, 3, 1, 2)))
        gemm = dict(A=A, s=np.repeat(rs.reshape(-1), W), W=w.reshape(Co, Ci * 9).numpy(), epi=epi, tap=np.arange(Ci * 9) % 9 == 5)
    elif kind == "tdf":
        B, C, T, K, N, resid = s["B"], s["C"], s["T"], s["K"], s["N"], s.get("resid", False)
        x = act((B, C, T, K), 3.0)
        w = wgt((N, K), K)
        sc, sh = tdf_scale(C), vec(C, 2, 0.3)
        t.update(x=x, w=w, scale=sc, shift=sh)
        lin = F.linear(x.double(), w.double())
        ref = F.relu(lin * _v(sc) + _v(sh))
        if resid:
            t["resid"] = _grid(rng, (B, C, T, N), xl) if exact else torch.randn(B, C, T, N, generator=g)
            ref = ref + t["resid"].double()
        if levels:
            in_amax = _blk_amax(x)
        rs = kernel_row_scale("tdf", None if in_amax is None else in_amax.numpy(), B, T)
        if exact:
            lo_x = _check_split(name + " x", x.numpy(), rs[:, None, :, None])
            lo_w = _check_split(name + " w", w.numpy(), CP.weight_scale(w.numpy()))
            assert not lo_x.any() or not lo_w.any(), f"{name}: xl*wl is not zero"
            lsb = _lsb(x) * _lsb(w)
            _check_sums(name, F.linear(x.abs().double(), w.abs().double()), lsb)
            _check_sums(name + " affine", F.linear(x.abs().double(), w.abs().double()) * _v(sc) + _v(sh).abs(), lsb * _lsb(sc))
        scn, shn = sc.numpy(), sh.numpy()
        rn = t["resid"].numpy() if resid else None

        def epi(acc):
            v = acc.reshape(B, C, T, N)
            v = np.maximum(v * scn[None, :, None, None] + shn[None, :, None, None], 0)
            return torch.from_numpy(np.ascontiguousarray(v + rn if rn is not None else v))
        tap = np.zeros(K, bool); tap[5] = True
        gemm = dict(A=x.reshape(-1, K).numpy(), s=np.repeat(rs[:, None, :], C, axis=1).reshape(-1), W=w.numpy(), epi=epi, tap=tap)
    elif kind in ("down", "up"):
        B, Ci, Co, H, W = s["B"], s["Ci"], s["Co"], s["H"], s["W"]
        x = act((B, Ci, H, W))
        bias = vec(Co, 3, 0.2)
        if levels:
            in_amax = _blk_amax(x)
        rs = kernel_row_scale(kind, None if in_amax is None else in_amax.numpy(), B, H)
        if kind == "down":
            w = wgt((Co, Ci, 2, 2), 4 * Ci)
            ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=2))
            abs_sum = F.conv2d(x.abs().double(), w.abs().double(), bias.abs().double(), stride=2)
            wm = w.reshape(Co, Ci * 4)
            Ho, Wo = H // 2, W // 2
            A = F.unfold(x, 2, stride=2).transpose(1, 2).reshape(B * Ho * Wo, Ci * 4).numpy()
            x_scale = np.repeat(rs, 2, axis=1)[:, None, :, None]
            bnp = bias.numpy()

            def epi(acc):
                v = np.maximum(acc + bnp[None, :], 0)
                return torch.from_numpy(np.ascontiguousarray(v.reshape(B, Ho, Wo, Co).transpose(0, 3, 1, 2)))
            gemm = dict(A=A, s=np.repeat(rs.reshape(-1), Wo), W=wm.numpy(), epi=epi, tap=np.arange(Ci * 4) % 4 == 1)
        else:
            w = wgt((Ci, Co, 2, 2), Ci)
            ref = F.relu(F.conv_transpose2d(x.double(), w.double(), bias.double(), stride=2))
            abs_sum = F.conv_transpose2d(x.abs().double(), w.abs().double(), bias.abs().double(), stride=2)
            wm = w.permute(1, 2, 3, 0).reshape(Co * 4, Ci)
            x_scale = rs[:, None, :, None]
            skn = None
            if s.get("skip", False):
                t["skip"] = _ints(rng, (B, Co, 2 * H, 2 * W), 2) if exact else torch.randn(B, Co, 2 * H, 2 * W, generator=g)
                ref = ref * t["skip"].double()
                skn = t["skip"].numpy()
            bnp = np.repeat(bias.numpy(), 4)

            def epi(acc):
                v = np.maximum(acc + bnp[None, :], 0).reshape(B, H, W, Co, 2, 2).transpose(0, 3, 1, 4, 2, 5).reshape(B, Co, 2 * H, 2 * W)
                return torch.from_numpy(np.ascontiguousarray(v * skn if skn is not None else v))
            tap = np.zeros(Ci, bool); tap[Ci // 2] = True
            gemm = dict(A=x.permute(0, 2, 3, 1).reshape(-1, Ci).numpy(), s=np.repeat(rs.reshape(-1), W), W=wm.numpy(), epi=epi, tap=tap)
        t.update(x=x, w=w, wm=wm.contiguous(), bias=bias)
        if exact:
            lo_x = _check_split(name + " x", x.numpy(), x_scale)
            lo_w = _check_split(name + " w", w.numpy(), CP.weight_scale(w.numpy()))
            assert not lo_x.any() or not lo_w.any(), f"{name}: xl*wl is not zero"
            _check_sums(name, abs_sum, _lsb(x, bias) * _lsb(w))
    elif kind == "tdf_small":
        B, C, T, Fq, Hd = s["B"], s["C"], s["T"], s["F"], s["Hd"]
        # two stages: h sits on the grid of stage 1's products, so stage 2 multiplies it by INTEGERS only, and both weights are
        # sparse enough that the second stage's sums stay below 2^24 of ITS grid step (asserted below on the actual h)
        x = act((B, C, T, Fq))
        if exact:
            w1 = _grid(rng, (Hd, Fq), wl, 2, density=min(1.0, 12.0 / Fq))
            w2 = _ints(rng, (Fq, Hd), 2) * torch.from_numpy((rng.random((Fq, Hd)) < min(1.0, 8.0 / Hd)).astype(np.float32))
            s1 = torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=C)); s2 = torch.from_numpy(rng.choice(np.array([1.0, 2.0, 3.0], np.float32), size=C))
            if C <= 3:                                          # every channel its own scale and shift
                s1 = torch.tensor([0.5, 1.0, 2.0][:C]); s2 = torch.tensor([1.0, 2.0, 3.0][:C])
                b1 = torch.tensor([1.0, -2.0, 3.0][:C]); b2 = torch.tensor([-1.0, 2.0, 0.0][:C])
            else:
                b1, b2 = vec(C, 3), vec(C, 3)
        else:
            w1 = torch.randn(Hd, Fq, generator=g) / np.sqrt(Fq); w2 = torch.randn(Fq, Hd, generator=g) / np.sqrt(Hd)
            s1 = torch.rand(C, generator=g) + 0.5; b1 = torch.randn(C, generator=g) * 0.3
            s2 = torch.rand(C, generator=g) + 0.5; b2 = torch.randn(C, generator=g) * 0.3
        t.update(x=x, w1=w1, w2=w2, s1=s1, b1=b1, s2=s2, b2=b2)
        xd = x.double()
        h = F.relu(F.linear(xd, w1.double()) * _v(s1) + _v(b1))
        ref = xd + F.relu(F.linear(h, w2.double()) * _v(s2) + _v(b2))
        if exact:
            lsb1 = _lsb(x) * _lsb(w1)
            a1 = F.linear(xd.abs(), w1.abs().double())
            _check_sums(name + " stage 1", a1, lsb1)
            _check_sums(name + " stage 1 affine", a1 * _v(s1) + _v(b1).abs(), lsb1 * _lsb(s1))
            _check_f32(name + " h", h)
            lsb2 = _lsb(h) * _lsb(w2)
            a2 = F.linear(h, w2.abs().double())
            _check_sums(name + " stage 2", a2, lsb2)
            _check_sums(name + " stage 2 affine + residual", a2 * _v(s2) + _v(b2).abs() + xd.abs(), min(lsb2 * _lsb(s2), _lsb(x)))
    else:       # conv1x1
        B, Ci, Co, P, relu = s["B"], s["Ci"], s["Co"], s["P"], s.get("relu", True)
        x = act((B, Ci, 1, P))
        w = wgt((Co, Ci), Ci)
        bias = vec(Co, 3, 1.0)
        t.update(x=x, w=w, bias=bias)
        ref = F.conv2d(x.double(), w.double().view(Co, Ci, 1, 1), bias.double())
        ref = F.relu(ref) if relu else ref
        if exact:
            _check_sums(name, F.conv2d(x.abs().double(), w.abs().double().view(Co, Ci, 1, 1), bias.abs().double()), _lsb(x, bias) * _lsb(w))
    if exact:
        _check_f32(name, ref)
    return Case(kind, s, grid, t, ref, in_amax, gemm)


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy emulation of the kernels' arithmetic
BREAKS = ("drop_xl_wh", "drop_xh_wl", "zero_tap", "skip_kstep", "swap_cols")


def split_gemm(A: np.ndarray, row_scale: np.ndarray, Wm: np.ndarray, brk: Optional[str] = None, tap: Optional[np.ndarray] = None) -> np.ndarray:
    """acc[m][n] = sum_k x[m][k] w[n][k] the way the split-f16 kernels form it: x scaled per row by a power of two, weights by
    conv_pack.weight_scale, both split into float16 hi / lo, k walked in steps of 32 with the three terms ah*bl, al*bh, ah*bh added to
    a float32 accumulator, the scales undone exactly at the end.  `brk`: one deliberate defect (BREAKS)."""
    A = np.asarray(A, np.float32); Wm = np.asarray(Wm, np.float32)
    ws = np.float32(CP.weight_scale(Wm))
    xh, xl = split16(A * np.asarray(row_scale, np.float32)[:, None])
    wh, wl = split16(Wm * ws)
    if brk == "zero_tap":
        xh = xh * ~tap[None, :]; xl = xl * ~tap[None, :]
    acc = np.zeros((A.shape[0], Wm.shape[0]), np.float32)
    k = A.shape[1]
    steps = list(range(0, k, 32))
    for i, k0 in enumerate(steps):
        if brk == "skip_kstep" and i == len(steps) // 2:
            continue
        sl = slice(k0, min(k, k0 + 32))
        if brk != "drop_xh_wl":
            acc += xh[:, sl] @ wl[:, sl].T
        if brk != "drop_xl_wh":
            acc += xl[:, sl] @ wh[:, sl].T
        acc += xh[:, sl] @ wh[:, sl].T
    acc = acc * (np.float32(1) / ws) * (np.float32(1) / np.asarray(row_scale, np.float32))[:, None]
    if brk == "swap_cols":
        acc[:, [0, 1]] = acc[:, [1, 0]]
    return acc


def emulate(case: Case, brk: Optional[str] = None) -> torch.Tensor:
    """The kernel's result for `case` as the emulation computes it (float64 tensor in the output's layout)."""
    assert brk is None or brk in BREAKS
    if case.kind in SPLIT_KINDS:
        gm = case.gemm
        return gm["epi"](split_gemm(gm["A"], gm["s"], gm["W"], brk, gm["tap"])).double()
    assert brk not in ("drop_xl_wh", "drop_xh_wl"), "the true-float32 kernels have no split"
    t = case.t

    def f32_gemm(A, Wm, broken):
        A = np.asarray(A, np.float32).copy(); Wm = np.asarray(Wm, np.float32)
        if broken and brk == "zero_tap":
            A[:, A.shape[1] // 2] = 0
        if broken and brk == "skip_kstep":
            k0 = 32 * ((A.shape[1] // 32) // 2)
            A[:, k0:k0 + 32] = 0
        acc = A @ Wm.T
        if broken and brk == "swap_cols" and acc.shape[1] > 1:
            acc[:, [0, 1]] = acc[:, [1, 0]]
        return acc
    if case.kind == "conv1x1":
        x = t["x"].numpy(); B, Ci, _, P = x.shape
        acc = f32_gemm(x.transpose(0, 2, 3, 1).reshape(-1, Ci), t["w"].numpy(), True) + t["bias"].numpy()[None, :]
        acc = np.maximum(acc, 0) if case.shapes.get("relu", True) else acc
        return torch.from_numpy(np.ascontiguousarray(acc.reshape(B, 1, P, -1).transpose(0, 3, 1, 2))).double()
    x = t["x"].numpy(); B, C, T, Fq = x.shape
    ch = lambda a: a.numpy()[None, :, None, None]
    h = f32_gemm(x.reshape(-1, Fq), t["w1"].numpy(), True).reshape(B, C, T, -1)
    h = np.maximum(h * ch(t["s1"]) + ch(t["b1"]), 0)
    y = f32_gemm(h.reshape(B * C * T, -1), t["w2"].numpy(), False).reshape(B, C, T, Fq)
    return torch.from_numpy(x + np.maximum(y * ch(t["s2"]) + ch(t["b2"]), 0)).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# the accepted-envelope cases of tests/test_unet_kernel_envelope_gpu.py: (id, kind, shapes, takes amax).  Every shape carries the
# reason its loads and stores stay inside the tensors (from the kernels' indexing).
def _conv_cases():
    out = []
    for kind, co in (("conv", 48), ("conv_s8", 48), ("conv_w96", 96)):
        c = lambda **kw: dict(dict(B=1, Ci=16, Co=co, H=8, W=32, relu=True), **kw)
        # all convs: a tile is 8 x 32 outputs, H % 8 == 0 and W % 32 == 0 so tiles cover the plane exactly; patch loads are aligned
        # float4 at x0 - 4 + 4 q guarded (plain) or clamped and zeroed (s8 / w96) by 0 <= gy < H, 0 <= gx < W with W % 4 == 0
        out += [
            (f"{kind}-one_tile-relu", kind, c()),                               # one workgroup per channel block: all four borders in it
            (f"{kind}-one_tile-norelu", kind, c(relu=False)),
            (f"{kind}-16x32-B3", kind, c(B=3, H=16)),                           # two tile rows; grid 3 x 2: no XCD swizzle
            (f"{kind}-8x64-B2-norelu", kind, c(B=2, W=64, relu=False)),         # two tile columns: bw = 2, one band
            (f"{kind}-W800", kind, c(W=800)),                                   # 25 tiles: w9 bw = 5 x 5 bands (plain: bw = 1); band * bw + t % bw < tiles_x
            (f"{kind}-W928", kind, c(W=928, relu=False)),                       # 29 tiles (prime): bw = 1, 29 bands
            (f"{kind}-ci48-B2", kind, c(B=2, Ci=48)),                           # plain: 3 blocks, unpaired tail; s8 / w96: C_in % 32 == 16, trailing group of two stages
            (f"{kind}-ci32-B2", kind, c(B=2, Ci=32, H=16, relu=False)),         # plain: one block pair; s8 / w96: one full group of four stages; grid 4
            (f"{kind}-16x64-B2-swizzle", kind, c(B=2, H=16, W=64)),             # grid 2 x 1 x 2 x 2 = 8: the XCD remap is on (a bijection of 0..7 onto the tiles)
        ]
    c = lambda **kw: dict(dict(B=2, Ci=32, Co=48, H=8, W=32, relu=True), **kw)
    out += [("conv-ci32_co48", "conv", c()),                                    # C_in != C_out: weights indexed [cob][cb], cob < C_out / 48
            ("conv-ci16_co96", "conv", c(Ci=16, Co=96))]                        # two channel blocks of one tile
    return [(i, k, s, True) for i, k, s in out]


def _first_cases():
    out = []
    for c0 in (1, 3, 4):
        for ci in (16, 48, 64):
            # the spectrogram loads read channels q < C0 only; s_first holds 5 * 64 floats for C_in <= 64; the rest is the s8 kernel
            out.append((f"first-c0_{c0}-ci{ci}-one_tile", "first", dict(B=1, C0=c0, Ci=ci, Co=48, H=8, W=32), True))
            out.append((f"first-c0_{c0}-ci{ci}-16x64-B2", "first", dict(B=2, C0=c0, Ci=ci, Co=48, H=16, W=64), True))
    return out


def _tdf_cases():
    c = lambda **kw: dict(dict(B=1, C=16, T=8, K=32, N=96, resid=False), **kw)
    # a tile is 16 channels x 8 time rows of one item (C % 16 == 0, T % 8 == 0: tiles cover the rows exactly), K % 32 == 0 stages,
    # N % 96 == 0 column blocks of 96 or 192: every row / column index is below M / N; weights are indexed [nb][stage], nb < N / BN
    return [(i, "tdf", s, True) for i, s in [
        ("tdf-min-N96", c()), ("tdf-min-N96-resid", c(resid=True)),                    # NT 3, one workgroup
        ("tdf-min-N192", c(N=192)), ("tdf-min-N192-resid", c(N=192, resid=True)),      # NT 6, one workgroup
        ("tdf-T16-B2", c(B=2, T=16, resid=True)),                                      # two time tiles per channel group
        ("tdf-K64", c(K=64)),                                                          # two stages: both weight buffers
        ("tdf-N288", c(N=288, resid=True)),                                            # NT 3, three column blocks
        ("tdf-nblk8-plain_order", c(N=1536, resid=True)),                              # n_nblk 8, n_mblk 1: ord_g = 8, ord_r = 1 (mb = chunk < n_mblk)
        ("tdf-nblk8-supergroups", c(T=128, N=1536)),                                   # n_mblk 16: 4 x 16 super-groups, a bijection of the 128 workgroups
        ("tdf-B3", c(B=3, resid=True)),                                                # grid 3: no XCD swizzle
    ]]


def _tdf_small_cases():
    out = []
    for f in (32, 96):
        for hd in (1, 5, 47, 48):
            # M = 32: one wave-tile (the other three waves of the workgroup leave at m0 >= M); k < 4 ceil(Hd / 4) <= 16 ceil(Hd / 16) columns
            # of the h tile are written before they are read; the packed weights hold ceil(Hd / 16) x F / 16 and F / 16 x ceil(Hd / 4) tiles
            out.append((f"tdf_small-F{f}-Hd{hd}-M32", "tdf_small", dict(B=1, C=4, T=8, F=f, Hd=hd), True))
    # C * T = 48: the channel changes inside a wave's 32 rows (c = (m / T) % C per row); no out_amax at this shape
    out.append(("tdf_small-B2-C3-T16-channel_mid_wave", "tdf_small", dict(B=2, C=3, T=16, F=32, Hd=12), False))
    out.append(("tdf_small-B3-C8-T8-F96-Hd24", "tdf_small", dict(B=3, C=8, T=8, F=96, Hd=24), True))     # 6 waves: two workgroups, the second half empty
    return out


def _resample_cases():
    d = lambda **kw: dict(dict(B=2, Ci=8, Co=96, H=16, W=32), **kw)
    u = lambda **kw: dict(dict(B=2, Ci=6, Co=24, H=2, W=64, skip=False), **kw)
    # down: (H/2)(W/2) % 128 == 0 pixels per image; a loader float4 starts at column 2 xo with xo even, so it ends at 2 xo + 3 <= W - 1;
    # channels s * 8 + c < C_in (C_in % 8 == 0); stores are masked by co < C_out; weights zero-padded to 96 columns and K % 32
    # up: H W % 128 == 0; loads are masked by ci < C_in; column n = 4 co + 2 dy + dx < 4 C_out (4 C_out % 96 == 0); a store float4
    # covers output columns 2 xx .. 2 xx + 3 with xx even <= W - 2
    return [
        ("down-ci8-co8", "down", d(Co=8), True),                                # one stage; 88 masked columns
        ("down-ci8-co96-B3", "down", d(B=3), True),                             # one full column block; grid 3
        ("down-ci8-co104", "down", d(Co=104), True),                            # second column block with 8 live channels
        ("down-ci16-co48-B1", "down", d(B=1, Ci=16, Co=48), True),              # two stages
        ("down-16x64-co104-swizzle", "down", d(H=16, W=64, Co=104), True),      # 2 items x 2 tiles x 2 column blocks = 8 workgroups: XCD remap on
        ("down-W4-H128", "down", d(H=128, W=4, Co=8), False),                   # Wo = 2: a 128-pixel tile spans 64 output rows
        ("down-W12-H128", "down", d(H=128, W=12, Co=8, B=1), False),            # (W / 2) % 4 != 0: P = 384, three tiles
        ("up-ci1-co24", "up", u(Ci=1), True),                                   # W = 64: a wave is exactly one row; last wave: row_b == row_a
        ("up-ci6-co48-skip", "up", u(Co=48, skip=True), True),                  # two column blocks
        ("up-ci20-co72-B3", "up", u(B=3, Ci=20, Co=72), True),                  # three column blocks; grid 9
        ("up-ci33-co24-skip", "up", u(Ci=33, skip=True), True),                 # two stages, the second with one live channel
        ("up-4x64-co48-swizzle", "up", u(H=4, Co=48, skip=True), True),         # 2 items x 2 tiles x 2 column blocks = 8 workgroups: XCD remap on
        ("up-W4-H32", "up", u(H=32, W=4), False),                               # a tile spans 32 input rows
        ("up-W96-H4-skip", "up", u(B=1, H=4, W=96, Ci=20, skip=True), True),    # waves straddle rows at offset 32; last wave on the last row
        ("up-W68-H32", "up", u(B=1, H=32, W=68, Ci=33, Co=48), True),           # straddles at every offset % 4; the wave on rows H - 2 | H - 1
    ]


def _conv1x1_cases():
    out = []
    for ci, co in ((8, 9), (9, 8), (1, 1), (8, 8)):
        for relu in (True, False):
            # one thread per pixel quad, i < P / 4 = 1; channels masked by c < C_in (C_in <= 8) or co < C_out (C_out <= 8)
            out.append((f"conv1x1-{ci}to{co}-P4-B3-{'relu' if relu else 'norelu'}", "conv1x1", dict(B=3, Ci=ci, Co=co, P=4, relu=relu), False))
    return out


CASES = _conv_cases() + _first_cases() + _tdf_cases() + _tdf_small_cases() + _resample_cases() + _conv1x1_cases()
FAMILY = {"conv": "conv3x3", "conv_s8": "conv3x3", "conv_w96": "conv3x3", "first": "conv3x3_first", "tdf": "tdf_linear",
          "down": "down2x", "up": "up2x", "tdf_small": "tdf_small", "conv1x1": "conv1x1"}


def grids_of(kind: str):
    return ("xlo", "wlo") if kind in SPLIT_KINDS or kind == "tdf_small" else ("both",)


_CACHE: Dict[tuple, Case] = {}


def case_of(case_id: str, grid: str, levels: bool = False) -> Case:
    """make_case for an entry of CASES, built once per session and shared (the tensors are never modified)."""
    key = (case_id, grid, levels)
    if key not in _CACHE:
        idx = [c[0] for c in CASES].index(case_id)
        _, kind, shapes, _ = CASES[idx]
        _CACHE[key] = make_case(kind, shapes, seed=1000 + 7 * idx + ("xlo", "wlo", "both", "gauss").index(grid), grid=grid, levels=levels)
    return _CACHE[key]
