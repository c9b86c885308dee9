"""The loader / exporter kernels at their edges: the three polyphase resamplers (ac_resample_poly, ac_resample_poly_segments,
ac_resample_poly_pcm16: one device function, ac_common.h `ac_polyphase_dot_wave`, and one host framing, `Context._resample_filter`)
against a float64 reference that uses the SAME taps (tests/resample_refs.py), and the two PCM converters (`pcm16()` inside
ac_resample_poly_pcm16, ac_pack_pcm24) on known-answer vectors.

No tolerance here is tuned.  A comparison is either exact (integers, single taps, powers of two, bytes) or
`resample_refs.assert_same_taps`: half a float32 ulp for the final rounding plus the float64 summation bound.  The oracle
comparisons of test_export_loader.py / test_kernels_edges_gpu.py keep their 2e-6, which covers the filter DESIGN difference only.
Float32 denormal OUTPUTS of the resampler are not examined: the scaling cases keep every nonzero output normal (and assert it).

The case table (RATIOS, case_lengths, SIGNALS, reference) is imported by tests/test_resample_refs_host.py, which proves on the CPU
that three off-by-one mutants of the kernel's index arithmetic cannot pass these comparisons."""
import functools
import math

import numpy as np
import pytest
import torch

import resample_refs as R
from audio_cut_amd._native import Context, NativeError, _check, _ptr, _stream
from audio_cut_amd.utils.audio_export import pcm_bytes_host

pytestmark = pytest.mark.gpu

# ---- the case table -------------------------------------------------------------------------------------------------------
# the product's two ratios, the four small ones of the issue's table, and an unreduced pair for the wrapper's gcd reduction
RATIOS = [(147, 160), (160, 441), (2, 1), (1, 2), (3, 7), (7, 3), (44100, 48000)]
PRODUCT_RATIOS = [(147, 160), (160, 441)]
SIGNALS = ("noise", "edge", "dc")


@functools.lru_cache(maxsize=None)
def product_filter(up, down):
    """(reduced up, reduced down, hfull float32, n_pre_remove, tpp): what `Context.resample_poly(x, up, down)` uploads."""
    g = math.gcd(up, down)
    u, d = up // g, down // g
    hfull, n_pre_remove = Context._resample_filter(u, d)
    assert hfull.dtype == np.float32
    return u, d, hfull, int(n_pre_remove), -(-hfull.size // u)


def case_lengths(up, down):
    """n in {1, 2, tpp - 1, tpp, tpp + 1, 3 tpp + 5}, and for r in (0, 1, 31) the first n whose output count exceeds one workgroup
    (32 outputs) and is r modulo 32, hence r % 8 in (0, 1, 7) modulo the wave's group of 8.  A ratio that cannot produce such a
    count has no such length: 2 / 1 gives even counts only."""
    u, d, _, _, tpp = product_filter(up, down)
    lens = [1, 2, tpp - 1, tpp, tpp + 1, 3 * tpp + 5]
    for r in (0, 1, 31):
        hit = [n for n in range(2, 64 * max(u, d)) if R.n_out_of(n, u, d) > 32 and R.n_out_of(n, u, d) % 32 == r]
        if hit:
            lens.append(hit[0])
    return lens


def signal(name, n, seed):
    """noise: Gaussian x 0.3.  edge: noise x 2^-10 with x[0] = x[n - 1] = 1, so that the first and the last sample dominate
    wherever they meet a tap, however small (the row ends are 2e-8 .. 7e-8).  dc: 1.0."""
    if name == "dc":
        return np.ones(n, dtype=np.float32)
    x = (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)
    if name == "edge":
        x *= np.float32(2.0 ** -10)
        x[0] = x[n - 1] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def reference(up, down, n, name, mutant=None):
    """(x, y64, mag) of one case, computed once and shared (read-only) by the tests that need it."""
    u, d, hfull, npr, _ = product_filter(up, down)
    x = signal(name, n, 1000 * u + d + n)
    y, mag = R.polyphase_ref64(x, u, d, hfull, npr, R.n_out_of(n, u, d), mutant=mutant)
    for a in (x, y, mag):
        a.setflags(write=False)
    return x, y, mag


def cases():
    for up, down in RATIOS:
        for n in case_lengths(up, down):
            for name in SIGNALS:
                yield up, down, n, name


# ---- ac_resample_poly with the product's filters ------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_poly_same_taps(hip_ctx, up, down):
    """Every length of the case table times noise / edge-weighted / DC against the same-taps float64 reference; the rows on the
    device are the reference's rows."""
    u, d, hfull, npr, tpp = product_filter(up, down)
    hd, npr_dev = hip_ctx._resample_filter_dev(u, d)
    hpad, _ = R.padded_taps(hfull, u)
    assert npr_dev == npr and np.array_equal(hd.cpu().numpy(), hpad.reshape(tpp, u).T.reshape(-1))
    worst, differ, total = 0.0, 0, 0
    for n in case_lengths(up, down):
        for name in SIGNALS:
            x, y, mag = reference(up, down, n, name)
            got = hip_ctx.resample_poly(hip_ctx.to_device(x.copy()), up, down).cpu().numpy()
            assert got.shape == y.shape == (R.n_out_of(n, u, d),)
            w, k = R.assert_same_taps(got, y, mag, tpp, label=f"{up}/{down} n={n} {name}", quiet=True)
            worst, differ, total = max(worst, w), differ + k, total + got.size
    print(f"resample_poly {up}/{down} (tpp {tpp}), lengths {case_lengths(up, down)}: worst error / bound {worst:.3f}, "
          f"{differ} of {total} differ from float32(y64)")
    assert worst <= 1.0


@pytest.mark.parametrize("up,down", PRODUCT_RATIOS)
def test_resample_poly_impulse_train_is_the_taps(hip_ctx, up, down):
    """`down` well-separated unit impulses: every output is one tap times 1.0 plus zeros, so it equals float32(tap) exactly, and the
    outputs together read every tap of the padded filter once (test_resample_refs_host.py proves the coverage)."""
    u, d, hfull, npr, tpp = product_filter(up, down)
    x, expected, idx = R.impulse_train(u, d, hfull, npr)
    got = hip_ctx.resample_poly(hip_ctx.to_device(x), up, down).cpu()
    bad = np.flatnonzero(got.numpy() != expected)
    print(f"impulse train {up}/{down}: {x.size} -> {expected.size} outputs, {int(np.count_nonzero(idx >= 0))} taps read, {bad.size} differ")
    assert torch.equal(got, torch.from_numpy(expected)), (int(bad[0]), R.tap_range(int(bad[0]), x.size, u, d, tpp, npr))


@pytest.mark.parametrize("up,down", PRODUCT_RATIOS + [(3, 7), (7, 3)])
def test_resample_poly_scales_by_powers_of_two(hip_ctx, up, down):
    """resample(x 2^60) == resample(x) 2^60 and the same for 2^-60, bit for bit: the float64 accumulation has no absolute floor and
    does not overflow.  Every nonzero output stays a normal float32 (asserted), so the final rounding scales exactly too;
    denormal outputs are out of scope."""
    u, d, _, _, tpp = product_filter(up, down)
    for name in ("noise", "edge"):
        x = signal(name, 3 * tpp + 5, 5)
        base = hip_ctx.resample_poly(hip_ctx.to_device(x), up, down).cpu().numpy()
        for e in (60, -60):
            sc = np.float32(2.0 ** e)
            want = base * sc
            nz = want[want != 0]
            assert np.all(np.abs(nz) >= 2.0 ** -126) and np.all(np.isfinite(want))
            got = hip_ctx.resample_poly(hip_ctx.to_device(x * sc), up, down).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, e, int(np.count_nonzero(got != want)))


def _poisoned(hip_ctx, segments, gap=777):
    """A device buffer of NaN holding the finite `segments` `gap` samples apart -> (buffer, offsets)."""
    total = gap + sum(len(s) + gap for s in segments)
    host = np.full(total, np.nan, dtype=np.float32)
    offs, at = [], gap
    for s in segments:
        host[at: at + len(s)] = s
        offs.append(at)
        at += len(s) + gap
    return hip_ctx.to_device(host), offs


@pytest.mark.parametrize("up,down", PRODUCT_RATIOS)
def test_resamplers_read_nothing_outside_the_signal(hip_ctx, up, down):
    """The signal lies in a buffer of NaN: one read outside [0, n) - even against a 3e-8 tap, even against a zero-padded one -
    makes an output NaN.  All three kernels, the segmented one with two segments and both bucket settings."""
    u, d, hfull, npr, tpp = product_filter(up, down)
    n = 3 * tpp + 5
    x, y, mag = reference(up, down, n, "noise")
    x2, y2, mag2 = reference(up, down, tpp + 1, "edge")
    buf, (o1, o2) = _poisoned(hip_ctx, [x, x2])
    got = hip_ctx.resample_poly(buf[o1: o1 + n], up, down).cpu().numpy()
    assert not np.any(np.isnan(got))
    R.assert_same_taps(got, y, mag, tpp, label=f"in NaN, float {up}/{down}")
    for bucket in (0, 4096):
        out, out_off, out_len = hip_ctx.resample_poly_segments(buf, [o1, o2], [n, tpp + 1], up, down, bucket=bucket)
        host = out.cpu().numpy()
        assert not np.any(np.isnan(host)) and out_len == [y.size, y2.size]
        R.assert_same_taps(host[int(out_off[0]): int(out_off[0]) + y.size], y, mag, tpp, label=f"in NaN, segment 0 bucket {bucket}")
        R.assert_same_taps(host[int(out_off[1]): int(out_off[1]) + y2.size], y2, mag2, tpp, label=f"in NaN, segment 1 bucket {bucket}")
        pad = np.ones(host.size, dtype=bool)
        for oo, ol in zip(out_off, out_len):
            pad[int(oo): int(oo) + ol] = False
        assert np.all(host[pad] == 0.0) and not np.any(np.signbit(host[pad]))
    clean = hip_ctx.resample_poly_pcm16(hip_ctx.to_device(x.copy()), up, down)
    assert np.array_equal(hip_ctx.resample_poly_pcm16(buf[o1: o1 + n], up, down), clean)
    assert np.array_equal(clean, pcm_bytes_host(got, "PCM_16")[0].view("<i2"))


@pytest.mark.parametrize("up,down", PRODUCT_RATIOS + [(2, 1), (1, 2)])
def test_resample_poly_one_nan_poisons_exactly_its_outputs(hip_ctx, up, down):
    """One NaN inside the signal: the outputs that are NaN are exactly those whose tap range meets it (zero-padded taps included:
    0 x NaN = NaN), the others hold the bound."""
    u, d, hfull, npr, tpp = product_filter(up, down)
    n = 3 * tpp + 5
    x = signal("noise", n, 9)
    x[n // 2] = np.nan
    y, mag = R.polyphase_ref64(x, u, d, hfull, npr, R.n_out_of(n, u, d))
    got = hip_ctx.resample_poly(hip_ctx.to_device(x), up, down).cpu().numpy()
    assert 0 < int(np.isnan(y).sum()) < y.size // 2
    R.assert_same_taps(got, y, mag, tpp, label=f"one NaN {up}/{down} ({int(np.isnan(y).sum())} NaN outputs)")


# ---- synthetic filters through the C ABI --------------------------------------------------------------------------------------
GUARD = 64          # bytes of 0xA5 behind every output buffer


def _rows_dev(hip_ctx, rows):
    """rows[p][t] -> the device layout hp[p * tpp + t]."""
    return hip_ctx.to_device(np.ascontiguousarray(rows, dtype=np.float32).reshape(-1))


def _abi_float(hip_ctx, xd, n, up, down, hd, npr, n_out):
    buf = torch.full((4 * n_out + GUARD,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    _check(hip_ctx.lib.ac_resample_poly(hip_ctx._h, _ptr(xd), n, up, down, _ptr(hd), hd.numel(), npr, _ptr(buf), n_out, _stream()))
    host = buf.cpu().numpy()
    assert np.all(host[4 * n_out:] == 0xA5)
    return host[: 4 * n_out].view(np.float32)


def _abi_segments(hip_ctx, xd, n, up, down, hd, npr, n_out):
    """The same input as two segments behind each other in the output."""
    buf = torch.full((8 * n_out + GUARD,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    i64 = lambda *v: hip_ctx.to_device(np.asarray(v, dtype=np.int64))
    d_io, d_il, d_oo, d_ol = i64(0, 0), i64(n, n), i64(0, n_out), i64(n_out, n_out)
    _check(hip_ctx.lib.ac_resample_poly_segments(hip_ctx._h, _ptr(xd), _ptr(d_io), _ptr(d_il), _ptr(d_oo), _ptr(d_ol), 2, up, down,
                                                 _ptr(hd), hd.numel(), npr, _ptr(buf), 2 * n_out, _stream()))
    host = buf.cpu().numpy()
    assert np.all(host[8 * n_out:] == 0xA5)
    return host[: 8 * n_out].view(np.float32).reshape(2, n_out)


def _abi_pcm16(hip_ctx, xd, n, up, down, hd, npr, n_out):
    padded = -(-n_out // 8) * 8
    buf = torch.full((2 * padded + GUARD,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    assert buf.data_ptr() % 16 == 0
    _check(hip_ctx.lib.ac_resample_poly_pcm16(hip_ctx._h, _ptr(xd), n, up, down, _ptr(hd), hd.numel(), npr, _ptr(buf), n_out, _stream()))
    host = buf.cpu().numpy()
    words = host[: 2 * padded].view("<i2")
    assert np.all(words[n_out:] == 0) and np.all(host[2 * padded:] == 0xA5)      # the last group is zero filled, nothing behind it
    return words[:n_out]


def _integer_ref(x, rows, up, down, npr, n_out):
    """The definition in integer arithmetic -> (y int64 [n_out], empty bool [n_out]: outputs with no tap in range)."""
    tpp = rows.shape[1]
    y = np.zeros(n_out, dtype=np.int64)
    empty = np.zeros(n_out, dtype=bool)
    for m in range(n_out):
        j0, p, t_lo, t_hi = R.tap_range(m, x.size, up, down, tpp, npr)
        empty[m] = t_lo > t_hi
        for t in range(t_lo, t_hi + 1):
            y[m] += int(rows[p, t]) * int(x[j0 - t])
    return y, empty


@pytest.mark.parametrize("tpp", [130, 4])
@pytest.mark.parametrize("npr", [0, 2])
def test_integer_filters_are_exact_in_all_three_kernels(hip_ctx, tpp, npr):
    """up 3, down 2, integer taps in [-3, 3] and integer samples in [-15, 15]: every partial sum is an integer below
    tpp * 45 < 2^24, exact in any order and any precision, so the float, segmented and pcm16 kernels must equal integer arithmetic
    bit for bit (pcm16 on x * 2^-15, where the PCM words ARE the integers).  tpp = 130 gives lanes 0 and 1 three taps and the other
    lanes two.  With 40 outputs more than ceil(n up / down) the tap range runs past the signal and, for tpp = 4, becomes empty:
    those outputs are +0.0 (not -0.0, not the 0xA5 the buffers are prefilled with)."""
    up, down = 3, 2
    rng = np.random.default_rng(10 * tpp + npr)
    rows = rng.integers(-3, 4, size=(up, tpp))
    hd = _rows_dev(hip_ctx, rows)
    seen_empty = 0
    for n in (1, 7, 129, 130, 131, 400):
        x = rng.integers(-15, 16, size=n)
        xd = hip_ctx.to_device(x.astype(np.float32))
        xd16 = hip_ctx.to_device((x * 2.0 ** -15).astype(np.float32))
        for extra in (0, 40):
            n_out = R.n_out_of(n, up, down) + extra
            want, empty = _integer_ref(x, rows, up, down, npr, n_out)
            assert np.max(np.abs(want)) < 2 ** 15
            seen_empty += int(empty.sum())
            flt = _abi_float(hip_ctx, xd, n, up, down, hd, npr, n_out)
            assert np.array_equal(flt, want.astype(np.float32)), (n, extra, int(np.argmax(flt != want)))
            assert not np.any(np.signbit(flt[empty])), (n, extra)
            seg = _abi_segments(hip_ctx, xd, n, up, down, hd, npr, n_out)
            assert np.array_equal(seg[0], want.astype(np.float32)) and np.array_equal(seg[1], want.astype(np.float32)), (n, extra)
            assert not np.any(np.signbit(seg[:, empty])), (n, extra)
            pcm = _abi_pcm16(hip_ctx, xd16, n, up, down, hd, npr, n_out)
            assert np.array_equal(pcm, want.astype(np.int16)), (n, extra, int(np.argmax(pcm != want)))
    print(f"integer filter tpp {tpp}, n_pre_remove {npr}: exact; {seen_empty} outputs with an empty tap range")
    assert (seen_empty > 0) == (tpp == 4)


# the PCM_16 known answers, hand-derived from libsndfile pcm.c f2les_clip_array (what soundfile.write runs): s = x * 2^31 in float32;
# s >= 0x7FFFFFFF -> 0x7FFF; s <= -2^31 -> 0x8000; NaN -> 0 (the product's choice: lrintf is undefined there); else
# lrintf(s) >> 16: half to even, then a FLOOR by 2^16.  TINY is the smallest float32 denormal; a tie (k + 0.5) 2^-31 has s = k + 0.5.
TINY = float(np.float32(2.0 ** -149))
T31 = 2.0 ** -31
PCM16_KAT = [
    (0.0, 0), (-0.0, 0), (1.0, 32767), (-1.0, -32768), (0.5, 16384), (-0.5, -16384), (1.5, 32767), (-1.5, -32768),
    (np.inf, 32767), (-np.inf, -32768), (np.nan, 0), (TINY, 0), (-TINY, 0),              # lrintf(-tiny) = -0 -> 0, not -1
    (1.0 - 2.0 ** -24, 32767),                 # s = 2^31 - 128 < 2^31: not clipped, (2^31 - 128) >> 16
    (-(1.0 - 2.0 ** -24), -32768),             # floor(-(2^31 - 128) / 2^16)
    (65535.5 * T31, 1),                        # 65535.5 -> 65536 (even) -> 1
    (65534.5 * T31, 0),                        # 65534.5 -> 65534 (even) -> 0
    (-65535.5 * T31, -1),                      # k = -65536: -65535.5 -> -65536 -> -1
    (-65536.5 * T31, -1),                      # k = -65537: -65536.5 -> -65536 (even) -> -1, not -2
    (0.5 * T31, 0), (-0.5 * T31, 0),           # +-0.5 -> +-0
    (0.9 * 2.0 ** -15, 0),                     # 58982.4 -> 58982 -> 0
    (-0.9 * 2.0 ** -15, -1),                   # -58982 -> floor -> -1
    (-0.1 * 2.0 ** -15, -1),                   # -6554 -> -1
]

# PCM_24: the 15 values of test_export_loader.py::test_pcm24_arithmetic_and_wav_round_trip with their answers, then -0.0, +-Inf, NaN,
# +-denormal and the ties (k + 0.5) 2^-31 for k in (255, 254, -256, -257, 0, -1): lrintf(s) >> 8
Q23 = 2.0 ** -23
PCM24_KAT = [
    (0.0, 0), (1.0, 8388607), (-1.0, -8388608), (0.5, 4194304), (-0.5, -4194304), (1.5, 8388607), (-1.5, -8388608), (1e-7, 0),
    (0.9 * Q23, 0), (-0.1 * Q23, -1), (1.0 - 2.0 ** -24, 8388607), (3.0 * Q23, 3), (-3.0 * Q23, -3), (2.5 * Q23, 2),
    (-(1.0 - Q23), -8388607),
    (-0.0, 0), (np.inf, 8388607), (-np.inf, -8388608), (np.nan, 0), (TINY, 0), (-TINY, 0),
    (255.5 * T31, 1),                          # 255.5 -> 256 (even) -> 1
    (254.5 * T31, 0),                          # 254.5 -> 254 (even) -> 0
    (-255.5 * T31, -1),                        # -256 -> -1
    (-256.5 * T31, -1),                        # -256 (even) -> -1, not -2
    (0.5 * T31, 0), (-0.5 * T31, 0),
]


def kat_arrays(kat):
    return np.array([v for v, _ in kat], dtype=np.float32), np.array([w for _, w in kat], dtype=np.int64)


def pcm24_bytes(words):
    w = np.asarray(words, dtype=np.int64) & 0xFFFFFF
    return np.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], axis=1).astype(np.uint8).reshape(-1)


def test_identity_filter_copies_and_converts(hip_ctx):
    """up = down = 1, hp = [1.0]: ac_resample_poly is a copy, bit for bit (+-0, denormals, +-Inf; NaN stays NaN), and
    ac_resample_poly_pcm16 is `pcm16()` alone: the known-answer vector at every rotation, lengths 1, 7, 8, 9 (a lone sample, one
    short of a 16-byte group, a whole group, one into the next), against the hand-derived words and against pcm_bytes_host."""
    one = _rows_dev(hip_ctx, [[1.0]])
    vals, words = kat_arrays(PCM16_KAT)
    x = np.concatenate([vals, np.float32([2.0 ** -126, -2.0 ** -126, 3.0 * TINY, 3.4028235e38, -3.4028235e38, 0.1, -1e-30])])
    got = _abi_float(hip_ctx, hip_ctx.to_device(x), x.size, 1, 1, one, 0, x.size)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan)
    same = got.view(np.uint32)[~nan] == x.view(np.uint32)[~nan]
    assert np.all(same), [(float(a), float(b)) for a, b in zip(x[~nan][~same], got[~nan][~same])]
    assert np.array_equal(pcm_bytes_host(vals, "PCM_16")[0].view("<i2"), words)
    for length in (1, 7, 8, 9):
        for r in range(vals.size):
            v, w = np.roll(vals, -r)[:length], np.roll(words, -r)[:length]
            pcm = _abi_pcm16(hip_ctx, hip_ctx.to_device(v), length, 1, 1, one, 0, length)
            assert np.array_equal(pcm, w), (length, r, v.tolist(), pcm.tolist(), w.tolist())


def test_resample_refusals_by_name(hip_ctx):
    """Both float entry points refuse bad sizes and null pointers with the message of the violated condition, and launch nothing."""
    lib, h = hip_ctx.lib, hip_ctx._h
    hd = _rows_dev(hip_ctx, np.ones((3, 4)))
    xd = hip_ctx.to_device(np.ones(16, dtype=np.float32))
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    i64 = lambda *v: hip_ctx.to_device(np.asarray(v, dtype=np.int64))
    io, il, oo, ol = i64(0), i64(16), i64(0), i64(16)
    X, H, O, S = _ptr(xd), _ptr(hd), _ptr(out), _stream()

    def refused(rc, name):
        with pytest.raises(NativeError, match=name):
            _check(rc)

    refused(lib.ac_resample_poly(h, X, 16, 3, 2, H, 11, 0, O, 16, S), r"polyphase rows \(hlen % up == 0")
    refused(lib.ac_resample_poly(h, X, 0, 3, 2, H, 12, 0, O, 16, S), "sizes must be positive")
    refused(lib.ac_resample_poly(h, X, 16, 3, 2, H, 12, 0, O, 0, S), "sizes must be positive")
    refused(lib.ac_resample_poly(h, X, 16, 3, 2, H, 12, -1, O, 16, S), "sizes must be positive")
    refused(lib.ac_resample_poly(h, None, 16, 3, 2, H, 12, 0, O, 16, S), "null pointer")
    refused(lib.ac_resample_poly(h, X, 16, 3, 2, None, 12, 0, O, 16, S), "null pointer")
    refused(lib.ac_resample_poly(h, X, 16, 3, 2, H, 12, 0, None, 16, S), "null pointer")
    seg = lambda x=X, a=_ptr(io), b=_ptr(il), c=_ptr(oo), d=_ptr(ol), n_seg=1, hp=H, hlen=12, npr=0, o=O, total=16: \
        lib.ac_resample_poly_segments(h, x, a, b, c, d, n_seg, 3, 2, hp, hlen, npr, o, total, S)
    refused(seg(hlen=11), r"polyphase rows \(hlen % up == 0")
    refused(seg(n_seg=0), "sizes must be positive")
    refused(seg(total=0), "sizes must be positive")
    refused(seg(npr=-1), "sizes must be positive")
    for null in ("x", "a", "b", "c", "d", "hp", "o"):
        refused(seg(**{null: None}), "null pointer")
    assert bool(torch.all(out == 0xA5))


# ---- ac_pack_pcm24 --------------------------------------------------------------------------------------------------------
def test_pack_pcm24_known_answers_in_every_lane_and_in_the_tail(hip_ctx):
    """The known-answer vector at all 27 rotations: with n = 27 every value visits every lane of the four-sample groups (positions
    0 .. 23) and the three-sample byte-wise tail; n = 25 and 26 give tails of one and two, n = 24 none.  Through the C ABI into a
    buffer of 0xA5: the bytes equal the hand-derived words and pcm_bytes_host, and nothing is written behind byte 3 n."""
    vals, words = kat_arrays(PCM24_KAT)
    assert vals.size == 27
    assert np.array_equal(pcm_bytes_host(vals, "PCM_24")[0], pcm24_bytes(words))
    for length in (27, 26, 25, 24):
        for r in range(vals.size if length != 24 else 1):
            v, w = np.roll(vals, -r)[:length], np.roll(words, -r)[:length]
            xd = hip_ctx.to_device(v)
            buf = torch.full((3 * length + GUARD,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
            _check(hip_ctx.lib.ac_pack_pcm24(hip_ctx._h, _ptr(xd), length, _ptr(buf), _stream()))
            host = buf.cpu().numpy()
            assert np.array_equal(host[: 3 * length], pcm24_bytes(w)), (length, r)
            assert np.all(host[3 * length:] == 0xA5), (length, r)
            assert np.array_equal(hip_ctx.pack_pcm24(xd), pcm24_bytes(w))


def test_pack_pcm24_refusals(hip_ctx):
    xd = hip_ctx.to_device(np.zeros(16, dtype=np.float32))
    buf = torch.full((64,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    assert xd.data_ptr() % 16 == 0 and buf.data_ptr() % 4 == 0
    lib, h, S = hip_ctx.lib, hip_ctx._h, _stream()
    for args, name in (((xd.data_ptr() + 4, 8, _ptr(buf)), "x 16-byte and out 4-byte aligned"),
                       ((_ptr(xd), 8, buf.data_ptr() + 1), "x 16-byte and out 4-byte aligned"),
                       ((_ptr(xd), 0, _ptr(buf)), "n must be positive")):
        with pytest.raises(NativeError, match=name):
            _check(lib.ac_pack_pcm24(h, *args, S))
    assert bool(torch.all(buf == 0xA5))
