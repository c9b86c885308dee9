"""Stage-by-stage parity of the Silero VAD kernels (audio_cut_amd/csrc/ac_vad.hip): `ac_silero_frontend`, `ac_silero_lstm` and
`ac_silero_out` called directly, each against the float64 staged reference of tests/silero_refs.py on the same inputs, at the
shapes where the kernels take another path (partial workgroups, the first-window flag, empty and one-window chunks, saturating
gates), then the three chained through `SileroHipVad.precompute`.

Tolerance rule of every numeric comparison, per launch:   max |kernel - ref64| <= 4 max |ref32 - ref64| + 2^-24 max |ref64|
ref32 is the float32 CPU evaluation of that one stage on the same inputs: it measures what float32 arithmetic costs on exactly this
case; 4 x is the margin tests/test_unet_gpu.py gives a kernel over a true float32 evaluation (another, fixed summation order stays
inside it, an arithmetic mistake does not), and the last term is half a float32 ulp of the largest value, for cases in which ref32
happens to round to ref64 (saturated or all-zero rows).  The output kernel yields ONE number per window, so a single window's
ref32 error is a sample of one; there the figure is taken over the nine windows of the case, of which every launch sees a prefix.

Worst kernel / ref32 error ratios per stage (the rule allows 4), as printed by these tests on an MI355X:

  stage / case                                              worst kernel error / ref32 error
  front end, silence, noise at 1e-6 and 1e-3, impulses      1.00 - 1.38    (6.2 - 8.7 before the bias of the gates was added last)
  front end, noise at 0.3, square wave, DC offset           2.38, 2.28, 2.06
  front end, flagged window after a loud chunk / at index 0 2.51
  LSTM, N(0, 1) gates x 1, 10, 50, 120                      0.95, 1.40, 0.85, 1.15
  LSTM, 2000 front-end steps                                0.87
  LSTM, chunks of 1, 0, 5, 1, 64 windows                    0.99           (a chunk's first window: 1.28)
  output layer, |h| <= 1 / rows of magnitude 50             2.63 / 1.00
  precompute chain, bucket 4096, 1000, 0                    1.00, 0.42, 1.00

The first line is a finding of these tests: `k_silero_frontend` started the 128-term sum of a gate at bias_ih + bias_hh (the
forget gate's is of order 1), so every small product was rounded at the bias's ulp: 8e-7 to 9e-7 on quiet input, where a float32
evaluation is off by 1.1e-7.  The kernel now adds the bias last.
"""
import numpy as np
import pytest
import torch

import silero_refs as R
from audio_cut_amd.testing.silero_synth import synth_silero_weights as base_weights

SR = 44100
F32, F64 = torch.float32, torch.float64
SENTINEL = np.float32(-12345.678)


# ---------------------------------------------------------------------------------------------------------------------
# shared helpers
# ---------------------------------------------------------------------------------------------------------------------
def check_rule(got, ref64, ref32, what, case=None):
    """The rule of the module docstring; prints the figures and returns kernel error / ref32 error.  `case` = (ref64, ref32) of the
    whole case where the launch sees only a part of it (the output kernel): the two figures of the bound are taken there."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape, ref32.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite kernel output"
    assert np.all(np.isfinite(ref64)) and np.all(np.isfinite(ref32)), f"{what}: non-finite reference"
    err = float(np.max(np.abs(got - ref64))) if got.size else 0.0
    c64, c32 = case if case is not None else (ref64, ref32)
    e32 = float(np.max(np.abs(c32.astype(np.float64) - c64))) if c64.size else 0.0
    bound = 4.0 * e32 + 2.0 ** -24 * (float(np.max(np.abs(c64))) if c64.size else 0.0)
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"[silero-rule] {what}: kernel {err:.3e}  ref32 {e32:.3e}  kernel/ref32 {ratio:.2f}  bound {bound:.3e}")
    assert err <= bound, f"{what}: |kernel - ref64| = {err:.3e} > {bound:.3e} (ref32 is off by {e32:.3e})"
    return ratio


def untouched(rows) -> bool:
    return bool(np.all(np.asarray(rows, dtype=np.float32).view(np.int32) == SENTINEL.view(np.int32)))


_PACKED = {}


def packed(ctx, key):
    """(numpy weights, device weights in kernel order) of a synthetic seed, or of ("cal", seed): the calibrated output layer."""
    if key not in _PACKED:
        from audio_cut_amd.detectors.silero_vad import SileroHipVad
        w = base_weights(key[1], affine=(60.0, -3.0)) if isinstance(key, tuple) else base_weights(key)
        _PACKED[key] = (w, SileroHipVad(SR, w, ctx)._pack())
    return _PACKED[key]


def run_frontend(ctx, p, x16_dev, win_start, extra=8):
    """-> gates_x [n, 512] on the host; `extra` sentinel rows behind them must come back untouched."""
    from audio_cut_amd._native import _check, _ptr, _stream
    n = len(win_start)
    gates = torch.full((n + extra, 512), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    d_ws = ctx.to_device(np.asarray(win_start, dtype=np.int64))
    _check(ctx.lib.ac_silero_frontend(ctx._h, _ptr(x16_dev), _ptr(d_ws), n, _ptr(p["basis_t"]), _ptr(p["c1"]), _ptr(p["b1"]),
                                      _ptr(p["c2"]), _ptr(p["b2"]), _ptr(p["c3"]), _ptr(p["b3"]), _ptr(p["c4"]), _ptr(p["b4"]),
                                      _ptr(p["wih_t"]), _ptr(p["bias_sum"]), _ptr(gates), _stream()))
    g = gates.cpu().numpy()
    assert untouched(g[n:]), f"front end wrote past row {n}"
    return g[:n]


def run_lstm(ctx, p, gates_dev, n_rows, seg_first, seg_count, extra=4):
    """-> h [n_rows + extra, 128] on the host, prefilled with the sentinel (rows no chunk owns must keep it)."""
    from audio_cut_amd._native import _check, _ptr, _stream
    hs = torch.full((n_rows + extra, 128), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    d_sf = ctx.to_device(np.asarray(seg_first, dtype=np.int32)); d_sc = ctx.to_device(np.asarray(seg_count, dtype=np.int32))
    _check(ctx.lib.ac_silero_lstm(ctx._h, _ptr(gates_dev), _ptr(d_sf), _ptr(d_sc), len(seg_first), _ptr(p["whh_t"]), _ptr(hs), _stream()))
    return hs.cpu().numpy()


def run_out(ctx, p, h_dev, n, extra=5):
    from audio_cut_amd._native import _check, _ptr, _stream
    probs = torch.full((n + extra,), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    _check(ctx.lib.ac_silero_out(ctx._h, _ptr(h_dev), _ptr(p["w_out"]), float(p["b_out"]), n, _ptr(probs), _stream()))
    pr = probs.cpu().numpy()
    assert untouched(pr[n:]), f"output kernel wrote past entry {n}"
    return pr[:n]


def one_chunk(n_windows, base=0):
    """win_start of one chunk at `base`: its first window flagged."""
    return [-(base) - 1] + [base + R.WINDOW * k for k in range(1, n_windows)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the staged reference is the network of the existing oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_staged_reference_equals_oracle():
    """The three float32 stages chained give `oracle.silero.silero_probs` within 2e-7 on 64 windows of noise at 0.3 (both are float32
    torch; they differ in batching only - measured 6e-8).  The float64 chain sits within 1e-6 of both."""
    from oracle import silero as OS
    w = base_weights(0)
    x = (0.3 * np.random.default_rng(11).standard_normal(64 * R.WINDOW)).astype(np.float32)
    want = OS.silero_probs(w, x)
    got = R.chain(w, x, one_chunk(64), [0], [64], F32)
    assert got.dtype == np.float32 and got.shape == want.shape == (64,)
    d = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"[silero-rule] staged float32 reference vs oracle: {d:.3e}")
    assert d <= 2e-7, d
    assert float(np.max(np.abs(R.chain(w, x, one_chunk(64), [0], [64], F64) - want))) < 1e-6
    # and the flag convention: the same position unflagged reads the 64 samples before it
    a = R.frontend_input(x, [-(1024) - 1], F64)[0]; b = R.frontend_input(x, [1024], F64)[0]
    assert torch.all(a[:64] == 0) and torch.equal(b[:64], torch.from_numpy(x[960:1024]).double()) and torch.equal(a[64:576], b[64:576])
    assert torch.equal(a[576:], torch.from_numpy(x[1024 + 447: 1024 + 511][::-1].copy()).double())       # reflected: samples 510 .. 447


# ---------------------------------------------------------------------------------------------------------------------
# front end
# ---------------------------------------------------------------------------------------------------------------------
FRONT_SIGNALS = ["zero", "noise_1e-6", "noise_1e-3", "noise_0.3", "square_1.0", "dc", "impulse_0", "impulse_511", "impulse_480"]
N_WINDOWS = (1, 7, 8, 9, 17)


def front_signal(kind, n_windows, seed):
    n = n_windows * R.WINDOW
    rng = np.random.default_rng(100 + seed)
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind.startswith("noise_"):
        return (float(kind[6:]) * rng.standard_normal(n)).astype(np.float32)
    if kind == "square_1.0":                                     # full scale, a period (74) that divides neither 128 nor 512
        return np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if kind == "dc":
        return (0.5 + 0.01 * rng.standard_normal(n)).astype(np.float32)
    x = np.zeros(n, np.float32)                                  # one impulse per window, at the same place of each
    x[int(kind[8:])::R.WINDOW] = 1.0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FRONT_SIGNALS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frontend_against_float64(hip_ctx, seed, kind):
    """gates_x of one chunk of 1, 7, 8, 9 and 17 windows (8 per workgroup: partial, full, full + 1, two full + 1) under the rule, for
    silence, noise from 1e-6 to 0.3, a full-scale square wave, a DC offset and an impulse at sample 0, at sample 511 and inside
    the reflected tail's source range (447 .. 510; at 480 and 511 it is also in the next window's context).  Rows behind
    n_windows keep their sentinel.  x16 is exactly n_windows * 512 long: nothing is read behind a window's 512 samples."""
    w, p = packed(hip_ctx, seed)
    x = front_signal(kind, max(N_WINDOWS), seed)
    ws = one_chunk(max(N_WINDOWS))
    ref64, ref32 = R.frontend(w, x, ws, F64), R.frontend(w, x, ws, F32)
    for n in N_WINDOWS:
        got = run_frontend(hip_ctx, p, hip_ctx.to_device(x[: n * R.WINDOW]), ws[:n])
        check_rule(got, ref64[:n], ref32[:n], f"frontend seed {seed} {kind} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frontend_first_window_flag(hip_ctx, seed):
    """win_start = -(index) - 1 means zero context.  Two chunks back to back with no gap: the first exactly 4096 samples and loud to
    its last sample, so the 64 samples before the second chunk's first window are NOT zeros; its gates must be those of the
    reference with zero context, which differ from the unflagged evaluation of the same position by far more than the tolerance
    (asserted: the case cannot pass vacuously).  The same for a flagged window at index 0 of the buffer the kernel is given, which
    here starts 64 samples into an allocation whose first 64 samples are loud."""
    w, p = packed(hip_ctx, seed)
    rng = np.random.default_rng(200 + seed)
    x = (0.5 * rng.standard_normal(4096 + 1024)).astype(np.float32)
    ws = one_chunk(8) + one_chunk(2, base=4096)
    ref64, ref32 = R.frontend(w, x, ws, F64), R.frontend(w, x, ws, F32)
    got = run_frontend(hip_ctx, p, hip_ctx.to_device(x), ws)
    check_rule(got, ref64, ref32, f"frontend seed {seed} two chunks, no gap")
    bound = 4.0 * float(np.max(np.abs(ref32[8] - ref64[8]))) + 2.0 ** -24 * float(np.max(np.abs(ref64[8])))
    unflagged = R.frontend(w, x, [4096], F64)[0]
    assert float(np.max(np.abs(unflagged - ref64[8]))) > 1000.0 * bound
    check_rule(got[8:9], ref64[8:9], ref32[8:9], f"frontend seed {seed} flagged window after a loud chunk")
    assert float(np.max(np.abs(got[8] - unflagged))) > 1000.0 * bound
    # index 0 of the buffer: the kernel gets the allocation + 64 samples
    xd = hip_ctx.to_device(x)
    got0 = run_frontend(hip_ctx, p, xd[64:], [-1, 512])
    r64, r32 = R.frontend(w, x, [-(64) - 1, 64 + 512], F64), R.frontend(w, x, [-(64) - 1, 64 + 512], F32)
    check_rule(got0, r64, r32, f"frontend seed {seed} flagged window at index 0")
    unflagged0 = R.frontend(w, x, [64], F64)[0]
    assert float(np.max(np.abs(unflagged0 - r64[0]))) > 1000.0 * bound and float(np.max(np.abs(got0[0] - unflagged0))) > 1000.0 * bound


@pytest.mark.gpu
def test_frontend_slot_independence(hip_ctx):
    """A window's gates do not depend on its slot in the 8-window workgroup, nor on its neighbours: the same 9 windows (two
    chunks, flagged and unflagged ones) behind 0 .. 7 dummy windows of other content give the same bits."""
    w, p = packed(hip_ctx, 0)
    rng = np.random.default_rng(300)
    x = np.concatenate([(0.3 * rng.standard_normal(9 * R.WINDOW)), np.where(np.arange(8 * R.WINDOW) % 50 < 25, 0.9, -0.9)]).astype(np.float32)
    xd = hip_ctx.to_device(x)
    ws = one_chunk(5) + one_chunk(4, base=5 * R.WINDOW)
    dummies = one_chunk(7, base=9 * R.WINDOW + 100)
    want = run_frontend(hip_ctx, p, xd, ws)
    check_rule(want, R.frontend(w, x, ws, F64), R.frontend(w, x, ws, F32), "frontend slot 0")
    for k in range(1, 8):
        got = run_frontend(hip_ctx, p, xd, dummies[:k] + ws)
        assert np.array_equal(got[k:].view(np.int32), want.view(np.int32)), f"{k} dummy windows in front change the bits"


# ---------------------------------------------------------------------------------------------------------------------
# LSTM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 10, 50, 120])
def test_lstm_synthetic_gates(hip_ctx, scale):
    """300 steps of N(0, 1) gates times 1, 10, 50 and 120 (the front end only ever produces |g| < 10): at 50 and 120
    `expf(-x)` overflows in the sigmoids and `tanhf` saturates; h stays finite, inside [-1, 1] and under the rule."""
    w, p = packed(hip_ctx, scale % 3)
    g = (scale * np.random.default_rng(400 + scale).standard_normal((300, 512))).astype(np.float32)
    if scale >= 50:
        assert float(np.max(np.abs(g))) > 89.0                  # expf overflows float32 above 88.7
    ref64, ref32 = R.lstm(w, g, [0], [300], F64), R.lstm(w, g, [0], [300], F32)
    h = run_lstm(hip_ctx, p, hip_ctx.to_device(g), 300, [0], [300])
    assert untouched(h[300:])
    assert float(np.max(np.abs(h[:300]))) <= 1.0
    check_rule(h[:300], ref64, ref32, f"lstm N(0,1) x {scale}, 300 steps")


@pytest.mark.gpu
def test_lstm_long_chunk(hip_ctx):
    """One chunk of 2000 windows of front-end gates (the float32 reference front end on noise whose level wanders between silence
    and 0.5): float32 error may accumulate along the recurrence, and must stay under the rule (float32 drift on the CPU: 4e-7)."""
    w, p = packed(hip_ctx, 0)
    n = 2000
    rng = np.random.default_rng(500)
    env = np.repeat(np.clip(np.cumsum(rng.standard_normal(n)) * 0.05 + 0.2, 0.0, 0.5), R.WINDOW)
    x = (env * rng.standard_normal(n * R.WINDOW)).astype(np.float32)
    g = R.frontend(w, x, one_chunk(n), F32)
    ref64, ref32 = R.lstm(w, g, [0], [n], F64), R.lstm(w, g, [0], [n], F32)
    h = run_lstm(hip_ctx, p, hip_ctx.to_device(g), n, [0], [n])
    assert untouched(h[n:])
    check_rule(h[:n], ref64, ref32, "lstm 2000 front-end steps")
    check_rule(h[n - 100: n], ref64[n - 100:], ref32[n - 100:], "lstm 2000 front-end steps, the last 100")


@pytest.mark.gpu
def test_lstm_chunk_layout(hip_ctx):
    """Chunks of 1, 0, 5, 1 and 64 windows in one launch (the empty one between real ones): every chunk starts from zero state
    (the reference resets it), the rows behind the last window keep their sentinel, and each chunk's h equals, bit for bit, the
    same chunk launched alone; an empty chunk launched alone writes nothing."""
    w, p = packed(hip_ctx, 1)
    counts = [1, 0, 5, 1, 64]
    firsts = [0, 1, 1, 6, 7]
    n = sum(counts)
    g = (3.0 * np.random.default_rng(600).standard_normal((n, 512))).astype(np.float32)
    gd = hip_ctx.to_device(g)
    ref64, ref32 = R.lstm(w, g, firsts, counts, F64), R.lstm(w, g, firsts, counts, F32)
    h = run_lstm(hip_ctx, p, gd, n, firsts, counts)
    assert untouched(h[n:])
    check_rule(h[:n], ref64, ref32, "lstm chunks 1, 0, 5, 1, 64")
    for f, c in zip(firsts, counts):
        if c:
            check_rule(h[f: f + 1], ref64[f: f + 1], ref32[f: f + 1], f"lstm first window of the chunk at {f}")
        alone = run_lstm(hip_ctx, p, gd, n, [f], [c])
        assert np.array_equal(alone[f: f + c].view(np.int32), h[f: f + c].view(np.int32)), (f, c)
        assert untouched(alone[:f]) and untouched(alone[f + c:]), (f, c)


# ---------------------------------------------------------------------------------------------------------------------
# output layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", [0, 1, 2, ("cal", 0)])
def test_out_against_float64(hip_ctx, key):
    """probs of 1, 3, 4, 5 and 9 windows (4 per workgroup) for h in the LSTM's range [-1, 1]: rows of mixed sign (the ReLU drops
    about half the terms) and all-negative rows (probability = sigmoid(bias)), either kind first; uncalibrated output layers and
    the calibrated one (logit times 60).  Entries behind n_windows keep their sentinel."""
    w, p = packed(hip_ctx, key)
    rng = np.random.default_rng(700)
    for phase in (0, 1):
        h = rng.uniform(-1.0, 1.0, (9, 128)).astype(np.float32)
        h[phase::2] = -np.abs(h[phase::2])
        hd = hip_ctx.to_device(h)
        ref64, ref32 = R.out(w, h, F64), R.out(w, h, F32)
        for n in (1, 3, 4, 5, 9):
            got = run_out(hip_ctx, p, hd, n)
            assert np.all((got >= 0) & (got <= 1))
            # the rule with the case's (nine windows') figures: one window is one number, see the module docstring
            check_rule(got, ref64[:n], ref32[:n], f"out weights {key} phase {phase} n={n}", case=(ref64, ref32))


@pytest.mark.gpu
def test_out_saturated(hip_ctx):
    """Outside the LSTM's range: rows of magnitude 50 against the calibrated layer drive the logit to several thousand of either
    sign, `expf` overflows: the result is finite, inside [0, 1] and under the rule (1 / (1 + inf) = 0 is the right answer)."""
    w, p = packed(hip_ctx, ("cal", 0))
    wo = w["decoder.decoder.2.weight"].reshape(128)
    h = np.stack([np.where(wo > 0, 50.0, -50.0), np.where(wo < 0, 50.0, -50.0), np.where(wo > 0, 50.0, -50.0),
                  np.full(128, -50.0), np.where(wo < 0, 50.0, -50.0)]).astype(np.float32)
    logit = np.maximum(h.astype(np.float64), 0) @ wo.astype(np.float64) + float(w["decoder.decoder.2.bias"][0])
    assert logit[0] > 100 and logit[1] < -100 and abs(logit[3] + 3.0) < 1e-6
    ref64, ref32 = R.out(w, h, F64), R.out(w, h, F32)
    got = run_out(hip_ctx, p, hip_ctx.to_device(h), 5)
    assert np.all(np.isfinite(got)) and np.all((got >= 0) & (got <= 1))
    check_rule(got, ref64, ref32, "out magnitude 50, calibrated")


# ---------------------------------------------------------------------------------------------------------------------
# the chain through the product path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calibrated():
    from silero_synth import synth_silero_weights
    return synth_silero_weights(0)


@pytest.fixture(scope="module")
def chain_chunks():
    """44.1 kHz chunks: 11 289 samples (exactly 4096 at 16 kHz) loud to the end, 9000 of voice, none, 200."""
    from audio_cut_amd.testing import signals
    rng = np.random.default_rng(800)
    loud = (0.4 * np.sin(2 * np.pi * 220.0 * np.arange(11289) / SR) + 0.2 * rng.standard_normal(11289)).astype(np.float32)
    return [loud, signals.voice_with_rests(1.0, seed=3)[:9000].astype(np.float32), np.zeros(0, np.float32),
            signals.c1_sine_silence(0.005, seed=1)[:200].astype(np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("bucket", [4096, 1000, 0])
def test_precompute_chain(hip_ctx, calibrated, chain_chunks, bucket):
    """`SileroHipVad.precompute` over [a chunk that fills its bucket exactly, a ragged one, an empty one, one shorter than a
    window] with the length bucket at 4096, 1000 and 0 (product and oracle configuration alike): lengths and window counts as
    oracle.silero, probabilities under the rule against the float64 chain fed with the product's own 16 kHz signal (so the
    resampler's float32 rounding stays out of the comparison), timestamps equal to the oracle's.  An empty chunk yields no window
    and no timestamp.  With bucket 4096 or 0 the second chunk's first window follows the loud tail of the first without a gap."""
    import math
    from audio_cut_amd import config as PCFG
    from audio_cut_amd.detectors.silero_vad import SileroHipVad
    from oracle import config as OCFG, silero as OS
    w = calibrated
    chunks = chain_chunks
    lens = [len(c) for c in chunks]
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1].tolist()
    saved = PCFG.snapshot()
    try:
        PCFG.set_runtime_config({"advanced_vad.silero_length_bucket": bucket})
        OCFG.set_runtime_config({"advanced_vad.silero_length_bucket": bucket})
        vad = SileroHipVad(SR, w, hip_ctx)
        packed_dev = hip_ctx.to_device(np.concatenate(chunks))
        pre = vad.precompute(packed_dev, offs, lens)
        assert len(pre) == len(chunks)
        # the product's own 16 kHz signal in the layout precompute uses
        step = math.lcm(bucket, R.WINDOW) if bucket > 0 else R.WINDOW
        x16, out_off, n16 = hip_ctx.resample_poly_segments(packed_dev, offs, lens, 160, 441, bucket=step)
        x16 = x16.cpu().numpy()
        ws, firsts, counts = [], [], []
        for c, p, off, m in zip(chunks, pre, out_off, n16):
            a16 = OS.resample_to_16k(c, SR) if len(c) else np.zeros(0, np.float32)
            padded = len(a16) + ((-len(a16)) % bucket if bucket > 0 else 0)
            n_win = len(OS.silero_probs(w, np.pad(a16, (0, padded - len(a16))))) if padded else 0
            assert (p.n, p.n16, p.n16_padded, len(p.probs)) == (len(c), len(a16), padded, n_win) and m == len(a16)
            firsts.append(len(ws)); counts.append(n_win)
            ws += one_chunk(n_win, base=int(off)) if n_win else []
            assert not np.any(x16[int(off) + len(a16): int(off) + n_win * R.WINDOW])       # the bucket padding is zeros
        assert counts[2] == 0 and counts[0] == (8 if bucket != 1000 else 10) and counts[3] >= 1
        if bucket != 1000:
            assert out_off[1] == 4096 and np.min(np.abs(x16[4096 - 64: 4096])) > 0            # no gap, and loud to the last sample
        ref64, ref32 = R.chain(w, x16, ws, firsts, counts, F64), R.chain(w, x16, ws, firsts, counts, F32)
        got = np.concatenate([p.probs for p in pre])
        assert got.dtype == np.float32 and np.all((got >= 0) & (got <= 1))
        check_rule(got, ref64, ref32, f"precompute chain bucket {bucket}")
        for c, p in zip(chunks, pre):
            want = OS.detect_speech_timestamps(c, SR, w) if len(c) else []
            assert vad(p) == want, (bucket, len(c), vad(p), want)
            assert vad(c) == want
    finally:
        PCFG.restore(saved)
        OCFG.reset_runtime_config()
