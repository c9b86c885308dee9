"""Framewise feature kernels (audio_cut_amd/csrc/ac_frames.hip) at their edges: signals shorter than a frame, one frame, a last block
of one frame, hop > frame, odd frames, frames at the LDS limits, windows cut by frame_lo / frame_hi, DC-only and Nyquist-only frames,
negative dB maxima, one-frame groups, 200 groups, median ties, every admitted tempogram window class, silent envelopes, YIN picks at
either end of the lag range and the one YIN shape that needs more than 64 KiB of LDS.  Each kernel is held to a plain float64
reference of the same operation (tests/frame_refs.py) through the `Context` wrappers; the references themselves are pinned against
oracle.librosa_ops on the CPU first.  Tolerances are those of tests/test_kernels_gpu.py for the same kernel.

Which test reaches which path:
  k_frame_rms        center=False, n < frame (refused), one frame, nf < fpb, one frame in the last block, hop > frame, hop 1, odd frame,
                     frame 15360 (fpb 1 and a 62 KiB span)                                  test_frame_rms_edges
                     frame > 15360, multi frame > 8192, more than four configurations      test_frame_rms_refusals_come_before_any_launch
  k_frame_rms_multi  n below one 8192-centre span at reach 4096, odd frames, frame 8192    test_frame_rms_multi_edges
  k_stft2048         n of 1 .. 2049, DC only, Nyquist only, single impulses                 test_stft2048_short_signals
                     windows cut, left with one sample or emptied by lo / hi, centres outside the signal, shuffled order, the 1e-10 clamp
                     on all-zero frames, flat-only and mel-only calls                      test_stft2048_grouped_windows_cut_by_their_bounds
  k_mel_group_max / k_onset_env
                     negative dB maximum, all-silent group, groups of 1 .. pad + 2 frames, 200 groups, median ranks among equal
                     values                                                                test_onset_strength_synthetic_mel
                     the song at 1e-2 and 1e-4 (maximum about -54 dB)                       test_onset_strength_quiet_song_end_to_end
  k_tempogram        win 2, 3, 160, 689, 1023, 1024; n of 1, 2, 63, 64, 65, 130, below win / 2, above win; silent envelope, -inf
                     prior, windows that are ramp but for 1 sample                               test_tempogram_reduce_edges
                     (no window lies wholly inside a ramp: a ramp is win / 2 long)
                     win 1 and 1025                                                        test_tempogram_reduce_refuses_windows_outside_2_to_1024
  k_yin              frames 64 .. 2048, three hops, two rates, n below one frame, picks at the first and the last lag, the
                     global-minimum path                                                   test_yin_f0_edges
                     a trough equal to its right neighbour                                 test_yin_f0_trough_on_an_exact_plateau
                     frame 4096, dynamic LDS above 64 KiB                                  test_yin_f0_frame_4096_needs_more_than_64_kib_of_lds
                     the `|b| >= |a|` guard cannot be reached through the entry point: an interior pick is strictly below its left
                     neighbour and not above its right one, so a > 0 and |b| <= a / 2.

What a one-token arithmetic change to a scratch copy of the kernel source did to this file on an MI355X:
  floor_db `- 80.0f` -> `- 79.0f`      fails test_onset_strength_synthetic_mel (6 of 8 cases), ..._quiet_song_end_to_end[1.0], [0.01]
  onset pad `1 +` -> `2 +`             fails every case of both onset tests
  far ramp `(p - 1 - r)` -> `(p - r)`  fails test_tempogram_reduce_edges at win 3, 160, 689, 1023, 1024 (at win 2 no window reaches it)
  trough `v <= right` -> `v < right`   fails test_yin_f0_trough_on_an_exact_plateau
  median `q < m` -> `q > m`            passes: equivalent, the ranks stay a permutation of 0 .. 127"""
import functools

import numpy as np
import pytest
import torch

import frame_refs as R
from audio_cut_amd import _native
from audio_cut_amd.testing import signals
from oracle import librosa_ops as L

SR = 44100
RMS_TOL = dict(rtol=2e-6, atol=1e-9)
STFT_TOL = dict(rtol=1e-4, atol=1e-12)
ONSET_TOL = dict(rtol=1e-4, atol=2e-5)
TG_TOL = dict(rtol=1e-9, atol=1e-12)
CMND_TOL = dict(rtol=1e-6, atol=1e-7)
TG_NEAR_TIE = 1e-7          # reference autocorrelation error (1e-13 relative, FFT against direct) times the largest slope of log1p(1e6 v)
TG_MAX_LEFT_OUT = 0.02


# ---------------------------------------------------------------------------------------------------------------------
# case builders (shared by the CPU pin test and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
RMS_CONFIGS = [(1, 1), (2, 1), (7, 3), (2205, 882), (1411, 1411), (441, 2000), (8191, 4096), (8192, 441), (15360, 15), (15360, 5000)]


def _rms_frames_per_block(frame, hop):
    """ac_frame_rms's own rule: as many frames as fit a 16 Ki-sample span, 1 .. 16."""
    return min(16, max(1, (16 * 1024 - frame) // hop + 1))


def _rms_lengths(frame, hop, center):
    pad = frame // 2 if center else 0
    one_in_last_block = frame - 2 * pad + _rms_frames_per_block(frame, hop) * hop         # fpb + 1 frames
    ns = [1, frame - 1, frame, frame + 1, frame + hop - 1, frame + hop, one_in_last_block]
    return sorted({n for n in ns if n >= 1})


def _rms_inputs(n, seed):
    rng = np.random.default_rng(seed)
    noise = (rng.standard_normal(n) * np.logspace(-9, 0, n)).astype(np.float32)
    first = np.zeros(n, np.float32); first[0] = 0.75
    last = np.zeros(n, np.float32); last[n - 1] = -0.5
    return {"noise": noise, "impulse_first": first, "impulse_last": last, "zeros": np.zeros(n, np.float32)}


STFT_LENGTHS = [1, 2, 441, 1023, 1024, 1025, 2047, 2048, 2049]
STFT_HOPS = [441, 512, 2205, 4096]


def _stft_inputs(n, seed):
    rng = np.random.default_rng(seed)
    out = {"noise": rng.standard_normal(n).astype(np.float32), "dc": np.full(n, 0.5, np.float32),
           "nyquist": (0.5 * (-1.0) ** np.arange(n)).astype(np.float32)}
    for pos in sorted({p for p in (0, 1, 1023, 1024, n - 1) if 0 <= p < n}):
        x = np.zeros(n, np.float32); x[pos] = 1.0
        out[f"impulse_{pos}"] = x
    return out


ONSET_HOPS = [441, 512, 2205, 4096]


def _onset_group(kind, length, rng):
    """One group's mel power [length, 128]."""
    if kind == "wide":                    # 1e-14 .. 1e6: values under amin and an active top_db clip
        return (10.0 ** rng.uniform(-14.0, 6.0, (length, 128))).astype(np.float32)
    if kind == "quiet":                   # maximum under 1.0: a negative dB maximum
        return (10.0 ** rng.uniform(-9.0, -1.0, (length, 128))).astype(np.float32)
    if kind == "zeros":
        return np.zeros((length, 128), np.float32)
    if kind == "ties":                    # 120 of the 128 bands share one value per row: 120 equal differences
        m = (10.0 ** rng.uniform(-3.0, 3.0, (length, 128))).astype(np.float32)
        bands = rng.permutation(128)[:120]
        m[:, bands] = (10.0 ** rng.uniform(-3.0, 3.0, (length, 1))).astype(np.float32)
        return m
    if kind == "flat":                    # every row the same: all differences zero
        return np.repeat((10.0 ** rng.uniform(-3.0, 3.0, (1, 128))).astype(np.float32), length, axis=0)
    raise ValueError(kind)


ONSET_KINDS = ["wide", "quiet", "zeros", "ties", "flat"]


def _onset_pool(hop, seed):
    pad = R.onset_pad(hop)
    rng = np.random.default_rng(seed)
    lengths = sorted({1, 2, pad, pad + 1, pad + 2, 23})
    return [(kind, n, _onset_group(kind, n, rng)) for kind in ONSET_KINDS for n in lengths]


TG_WINS = [2, 3, 160, 689, 1023, 1024]
TG_HOP = 512


def _tg_lengths(win):
    ns = {1, 2, 63, 64, 65, 130, win + 6}
    if win // 2 > 1:
        ns.add(max(1, win // 2 - 3))      # n < win // 2: the whole envelope is shorter than one ramp
    return sorted(ns)


def _tg_envelopes(n, seed):
    rng = np.random.default_rng(seed)
    dense = (0.05 + np.abs(rng.standard_normal(n))).astype(np.float32)
    sparse = (np.abs(rng.standard_normal(n)) * (rng.random(n) < 0.3)).astype(np.float32)
    first = np.zeros(n, np.float32); first[0] = 2.0
    last = np.zeros(n, np.float32); last[n - 1] = 2.0
    return {"dense": dense, "sparse": sparse, "constant": np.full(n, 0.7, np.float32), "spike_first": first, "spike_last": last,
            "zeros": np.zeros(n, np.float32)}


def _tg_logprior(win):
    """librosa.feature.tempo's prior, built as tests/test_kernels_gpu.py builds it."""
    bpms = L.tempo_frequencies(win, hop_length=TG_HOP, sr=SR)
    with np.errstate(divide="ignore"):
        logprior = -0.5 * ((np.log2(bpms) - np.log2(120.0)) / 1.0) ** 2
    logprior[: int(np.argmax(bpms < 320.0))] = -np.inf
    return logprior


@functools.lru_cache(maxsize=None)
def _tg_case(win, n, kind):
    """(envelope, reference tempogram mean, reference argmax, frames that may be left out) for the usual prior."""
    env = _tg_envelopes(n, seed=1000 * win + n)[kind]
    tg = R.tempogram_direct(env, win)
    score = np.log1p(1e6 * tg) + _tg_logprior(win)[:, None]
    arg = np.argmax(score, axis=0)
    top2 = np.sort(score, axis=0)[-2:]
    with np.errstate(invalid="ignore"):
        near = (top2[1] - top2[0]) < TG_NEAR_TIE          # -inf - -inf = nan compares False: a frame of -inf scores expects lag 0
    return env, tg.mean(axis=1), arg, near


def _tone(n, sr, period, harmonics=(1.0,)):
    t = np.arange(n, dtype=np.float64)
    return sum((0.4 * a / (h + 1)) * np.sin(2.0 * np.pi * (h + 1) * t / period + 0.3 * h) for h, a in enumerate(harmonics)).astype(np.float32)


YIN_RANGES = {"music": (44100, 65.40639132514966, 2093.004522404789),       # min_period 21; max_period clamped by short frames
              "speech_open": (16000, 50.0, 16000.0)}                         # min_period 1


def _yin_signals(n, sr, fmin, fmax, frame_length, seed):
    lo, hi = R.yin_periods(sr, fmin, fmax, frame_length)
    rng = np.random.default_rng(seed)
    mid = 0.5 * (lo + hi) + 0.3
    stop = _tone(n, sr, mid, (1.0, 0.6, 0.3))
    stop[(2 * n) // 3 + 5:] = 0.0
    return {"harmonic": _tone(n, sr, mid, (1.0, 0.6, 0.3)),
            "first_lag": _tone(n, sr, float(lo)) if lo > 1 else np.full(n, 0.25, np.float32),
            "last_lag": _tone(n, sr, float(hi)),
            "noise": (0.3 * rng.standard_normal(n)).astype(np.float32),
            "silence": np.zeros(n, np.float32),
            "stops": stop}


def _yin_lengths(frame_length):
    return [1, 100, frame_length - 1, frame_length, 3 * frame_length + 17]


YIN_PLATEAU = dict(sr=16000, fmin=50.0, fmax=8000.0, frame_length=64, hop=64, threshold=1.5)      # lags 2 .. 31


def _yin_plateau_signals():
    """Sparse impulses of +-0.5: every sum in the difference function is exact, and wherever d[tau] equals the running mean of
    d[1 .. tau] twice in a row cmnd is exactly 1.0 at both lags.  With the threshold at 1.5 such a pair can be the first trough:
    below its left neighbour and EQUAL to its right one."""
    out = {}
    for seed in (22, 32, 48, 71):
        rng = np.random.default_rng(seed)
        out[f"impulses_{seed}"] = (rng.integers(-1, 2, 320) * (rng.random(320) < (0.08, 0.15, 0.3)[seed % 3]) * 0.5).astype(np.float32)
    return out


def _first_trough(c, threshold, strict):
    """The trough rule on one cmnd row, as librosa states it (`strict` False) or with the right-hand `<=` turned into `<`."""
    for i in range(len(c)):
        left = c[i] < c[i - 1] if i > 0 else True
        right = True if i == len(c) - 1 else (c[i] < c[i + 1] if strict or i == 0 else c[i] <= c[i + 1])
        if left and right and c[i] < threshold:
            return i
    return int(np.argmin(c))


def _plateau_frames(cmnd, threshold):
    """Frames whose first trough sits on an exact plateau (equal to its right neighbour): the strict rule picks another lag."""
    out = []
    for f, c in enumerate(cmnd):
        i = _first_trough(c, threshold, False)
        if 0 < i < len(c) - 1 and c[i] < c[i - 1] and c[i] == c[i + 1] and c[i] < threshold and _first_trough(c, threshold, True) != i:
            out.append(f)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the references against the oracle, and the near-tie cap on the tempogram inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_references_match_the_oracle():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(6000) * np.logspace(-4, 0, 6000)).astype(np.float32)
    for frame, hop, center in [(7, 3, True), (2205, 882, True), (1411, 1411, False), (441, 2000, True), (2048, 441, True), (4410, 2205, False)]:
        ref = L.rms(x, frame_length=frame, hop_length=hop, center=center)[0]
        got = R.rms_direct(x, frame, hop, center)
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, **RMS_TOL)
    for n, hop in [(3000, 441), (5000, 2205), (700, 512)]:
        y = rng.standard_normal(n).astype(np.float32)
        ref_flat = L.spectral_flatness(y, hop_length=hop)[0]
        ref_mel = L.melspectrogram(y, SR, hop_length=hop, fmax=0.5 * SR).T
        got = [R.stft_frame_direct(y, f * hop) for f in range(1 + n // hop)]
        assert len(got) == len(ref_flat)
        np.testing.assert_allclose([g[0] for g in got], ref_flat, **STFT_TOL)
        np.testing.assert_allclose(np.array([g[1] for g in got]), ref_mel, **STFT_TOL)
    y = (rng.standard_normal(30000) * np.linspace(0.01, 1.0, 30000)).astype(np.float32)
    for hop in ONSET_HOPS:
        mel = L.melspectrogram(y, SR, hop_length=hop, fmax=0.5 * SR).T
        for agg, fn in (("mean", np.mean), ("median", np.median)):
            ref = L.onset_strength(y, sr=SR, hop_length=hop, aggregate=fn)
            got = R.onset_from_mel(mel, hop, agg)
            assert got.shape == ref.shape
            np.testing.assert_allclose(got, ref, **ONSET_TOL)
    for win, n in [(689, 700), (1024, 130), (160, 65), (3, 64), (2, 1), (1023, 40)]:
        env = np.abs(rng.standard_normal(n)).astype(np.float32)
        ref = L.tempogram(env, win)
        got = R.tempogram_direct(env, win)
        assert got.shape == ref.shape
        np.testing.assert_allclose(got.mean(axis=1), ref.mean(axis=1), **TG_TOL)
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
        assert np.array_equal(R.ramp_padded(env, win // 2), np.pad(env, (win // 2,) * 2, mode="linear_ramp", end_values=[0, 0]))
    for frame_length, hop, key in [(2048, 441, "music"), (1024, 128, "speech_open"), (64, 512, "music"), (64, 128, "speech_open")]:
        sr, fmin, fmax = YIN_RANGES[key]
        for name, y in _yin_signals(3 * frame_length + 17, sr, fmin, fmax, frame_length, seed=5).items():
            ref, lo, hi = L.cmnd_frames(y, sr, fmin, fmax, frame_length, hop)
            assert (lo, hi) == R.yin_periods(sr, fmin, fmax, frame_length)
            if name == "first_lag" and lo == 1:
                # a constant: inside it the difference function is exactly 0 when summed directly (all terms are exact in float32
                # and float64 alike), while the oracle's FFT leaves 1e-14 there and divides that by its own running mean.  Not a
                # case for the oracle.  What the direct sum must give is pinned instead: exactly 0 at every lag on the frames that lie
                # wholly inside the constant (and at the short lags of a frame that lies partly inside it), the oracle's value at its
                # tolerance wherever the direct sum is not exactly 0.
                got = R.cmnd_direct(y, sr, fmin, fmax, frame_length, hop)
                centres = np.arange(got.shape[0]) * hop
                inside = (centres - frame_length // 2 >= 0) & (centres + frame_length // 2 <= len(y))
                assert inside.sum() >= 1 and not got[inside].any()
                assert (got != 0.0).any()
                np.testing.assert_allclose(got[got != 0.0], ref.T[got != 0.0], err_msg=name, **CMND_TOL)
                continue
            got = R.cmnd_direct(y, sr, fmin, fmax, frame_length, hop)
            assert got.shape == ref.T.shape
            np.testing.assert_allclose(got, ref.T, err_msg=name, **CMND_TOL)
            ref_f0 = L.yin(y, fmin, fmax, sr=sr, frame_length=frame_length, hop_length=hop)
            np.testing.assert_allclose(sr / R.yin_pick(ref.T, lo, 0.1), ref_f0, rtol=1e-12, err_msg=name)
    # the selection rules on a hand-made series: a trough at the last lag, one at the first, a plateau (the first of equal minima)
    cm = np.array([[1.0, 0.9, 0.5, 0.3, 0.05], [0.05, 0.3, 0.5, 0.9, 1.0], [1.0, 0.5, 0.5, 0.5, 1.0], [1.0, 0.4, 0.04, 0.06, 1.0]])
    assert np.array_equal(R.yin_pick(cm, 10, 0.1)[:3], [14.0, 10.0, 11.5])
    assert R.yin_pick(cm, 10, 0.1)[3] == 12.0 - ((0.06 - 0.4) / 2.0) / (0.06 + 0.4 - 0.08)


def test_tempogram_inputs_stay_clear_of_near_ties():
    """The argmax comparison may leave out a frame whose best two reference scores are closer than 1e-7; the chosen inputs need that
    for at most 2 % of a case's frames, by themselves."""
    for win in TG_WINS:
        for n in _tg_lengths(win):
            for kind in _tg_envelopes(1, 0):
                near = _tg_case(win, n, kind)[3]
                assert near.sum() <= TG_MAX_LEFT_OUT * n, (win, n, kind, int(near.sum()))


def test_yin_plateau_inputs_have_a_plateau_at_their_first_trough():
    q = YIN_PLATEAU
    lo, _ = R.yin_periods(q["sr"], q["fmin"], q["fmax"], q["frame_length"])
    for name, x in _yin_plateau_signals().items():
        got = R.cmnd_direct(x, q["sr"], q["fmin"], q["fmax"], q["frame_length"], q["hop"])
        ref, _, _ = L.cmnd_frames(x, q["sr"], q["fmin"], q["fmax"], q["frame_length"], q["hop"])
        np.testing.assert_allclose(got, ref.T, err_msg=name, **CMND_TOL)
        assert _plateau_frames(got, q["threshold"]), name


def test_yin_voiced_cases_have_enough_clear_frames():
    for frame_length in (64, 1024, 2048, 4096):
        for key in YIN_RANGES:
            sr, fmin, fmax = YIN_RANGES[key]
            y = _yin_voiced(sr, fmin, fmax, frame_length)
            for hop in (128, 441, 512):
                ref, _, _ = L.cmnd_frames(y, sr, fmin, fmax, frame_length, hop)
                assert (ref.min(axis=0) < 0.05).sum() >= 20, (frame_length, key, hop)


def _yin_voiced(sr, fmin, fmax, frame_length):
    """The steady harmonic tone, long enough for 20 clearly periodic frames at every hop used here."""
    return _yin_signals(3 * frame_length + 40 * 512, sr, fmin, fmax, frame_length, seed=9)["harmonic"]


# ---------------------------------------------------------------------------------------------------------------------
# frame_rms / frame_rms_multi
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("frame,hop", RMS_CONFIGS)
def test_frame_rms_edges(hip_ctx, monkeypatch, frame, hop, center):
    pad = frame // 2 if center else 0
    for n in _rms_lengths(frame, hop, center):
        for name, x in _rms_inputs(n, seed=frame + hop + n).items():
            xd = hip_ctx.to_device(x)
            if n + 2 * pad < frame:                       # refused by the wrapper: the library is not even called
                with monkeypatch.context() as mp:
                    mp.setattr(hip_ctx.lib, "ac_frame_rms", lambda *a: pytest.fail("ac_frame_rms called"), raising=False)
                    with pytest.raises(_native.NativeError, match="shorter than one frame"):
                        hip_ctx.frame_rms(xd, frame, hop, center=center)
                continue
            got = hip_ctx.frame_rms(xd, frame, hop, center=center).cpu().numpy()
            ref = R.rms_direct(x, frame, hop, center)
            assert got.shape == ref.shape == (1 + (n + 2 * pad - frame) // hop,), (n, name)
            np.testing.assert_allclose(got, ref, err_msg=f"n={n} {name}", **RMS_TOL)
            assert np.array_equal(got == 0.0, ref == 0.0), (n, name)          # exact-zero frames stay exact zeros
            if name.startswith("impulse"):                 # one sample: exactly the frames that hold it are non-zero
                assert np.count_nonzero(got) == np.count_nonzero(ref)


@pytest.mark.gpu
def test_frame_rms_refusals_come_before_any_launch(hip_ctx):
    """The size limits are `AC_REQUIRE`s in front of the launch: the error names the requirement, and the stream stays usable."""
    x = hip_ctx.to_device(np.ones(40000, np.float32))
    for center in (True, False):
        with pytest.raises(_native.NativeError, match="invalid argument: frame too large for the LDS span"):
            hip_ctx.frame_rms(x, 15361, 441, center=center)
    with pytest.raises(_native.NativeError, match="invalid argument: frame too large for the LDS span"):
        hip_ctx.frame_rms_multi(x, [(2205, 882), (8193, 441)])
    with pytest.raises(_native.NativeError, match="invalid argument"):
        hip_ctx.frame_rms_multi(x, [(2205, 882)] * 5)
    torch.cuda.synchronize()
    assert hip_ctx.frame_rms(x, 15360, 441).cpu().numpy()[40] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 100, 8191, 8192, 8193])
def test_frame_rms_multi_edges(hip_ctx, n):
    """Every admitted configuration with frame <= 8192, in groups of 1 to 4: the same bits as the single kernel, which in turn
    matches the float64 reference at these lengths (shorter than, equal to and one past the 8192-centre span)."""
    cfgs = [c for c in RMS_CONFIGS if c[0] <= 8192]
    for name, x in _rms_inputs(n, seed=n).items():
        xd = hip_ctx.to_device(x)
        single = {}
        for frame, hop in cfgs:
            single[(frame, hop)] = hip_ctx.frame_rms(xd, frame, hop)
            np.testing.assert_allclose(single[(frame, hop)].cpu().numpy(), R.rms_direct(x, frame, hop, True), err_msg=f"{frame} {hop} {name}", **RMS_TOL)
        for k in (1, 2, 3, 4):
            for start in range(len(cfgs)):
                group = [cfgs[(start + 3 * j) % len(cfgs)] for j in range(k)]
                got = hip_ctx.frame_rms_multi(xd, group)
                for cfg, g in zip(group, got):
                    assert g.shape == single[cfg].shape and torch.equal(g, single[cfg]), (n, name, group, cfg)


# ---------------------------------------------------------------------------------------------------------------------
# stft2048_features
# ---------------------------------------------------------------------------------------------------------------------
def _check_stft_frames(x, frames, flat, mel):
    """frames: (centre, lo, hi) per row.  A frame with no energy at all must give flatness exactly 1 and mel exactly 0."""
    for f, (c, lo, hi) in enumerate(frames):
        ref_flat, ref_mel, power = R.stft_frame_direct(x, c, lo, hi)
        if not power.any():
            assert flat[f] == 1.0 and not mel[f].any(), (f, c, lo, hi)
        np.testing.assert_allclose(flat[f], ref_flat, err_msg=str((f, c, lo, hi)), **STFT_TOL)
        np.testing.assert_allclose(mel[f], ref_mel, err_msg=str((f, c, lo, hi)), **STFT_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("hop", STFT_HOPS)
def test_stft2048_short_signals(hip_ctx, hop):
    for n in STFT_LENGTHS:
        for name, x in _stft_inputs(n, seed=n + hop).items():
            flat, mel = hip_ctx.stft2048_features(hip_ctx.to_device(x), hop, want_flat=True, want_mel=True)
            nf = 1 + n // hop
            assert flat.shape == (nf,) and mel.shape == (nf, 128), (n, name)
            if name == "noise":
                assert len(L.spectral_flatness(x, hop_length=hop)[0]) == nf
            _check_stft_frames(x, [(f * hop, 0, n) for f in range(nf)], flat.cpu().numpy(), mel.cpu().numpy())


@pytest.mark.gpu
def test_stft2048_grouped_windows_cut_by_their_bounds(hip_ctx):
    n = 5000
    rng = np.random.default_rng(21)
    x = rng.standard_normal(n).astype(np.float32)
    frames = [(2500, 2400, 2600), (2500, 0, 2500), (2500, 2500, n), (2500, 1477, 3523),          # cut in the middle
              (2500, 2500, 2501), (2500, 1476, 1477), (2500, 1477, 1478), (2500, 3523, 3524),    # one sample (1476: under Hann's zero)
              (2500, 2500, 2500), (2500, 0, 1476), (2500, 3524, n), (2500, 0, 0), (2500, n, n),  # nothing
              (-500, 0, n), (-1023, 0, n), (-1024, 0, n), (-4000, 0, n),                         # centres before the signal
              (n + 600, 0, n), (n + 1023, 0, n), (n + 1024, 0, n), (n + 9000, 0, n),             # and past it
              (0, 0, n), (n, 0, n), (n - 1, 0, n), (1024, 0, n), (1024, 0, 2048), (1024, 1, 2047)]
    order = rng.permutation(len(frames))
    frames = [frames[i] for i in order] + frames                   # shuffled, then in order: a frame never depends on its position
    fc, lo, hi = (hip_ctx.to_device(np.array([fr[k] for fr in frames], dtype=np.int64)) for k in range(3))
    xd = hip_ctx.to_device(x)
    flat, mel = hip_ctx.stft2048_features(xd, 441, want_flat=True, want_mel=True, frame_center=fc, frame_lo=lo, frame_hi=hi)
    assert flat.shape == (len(frames),) and mel.shape == (len(frames), 128)
    _check_stft_frames(x, frames, flat.cpu().numpy(), mel.cpu().numpy())
    silent = [f for f, (c, a, b) in enumerate(frames) if b <= a or b <= c - 1024 or a >= c + 1024]
    assert len(silent) >= 2 * 9
    assert all(flat[f].item() == 1.0 and not mel[f].any().item() for f in silent)
    half = len(frames) // 2
    back = torch.as_tensor(np.argsort(order), device=flat.device)
    assert torch.equal(flat[:half][back], flat[half:]) and torch.equal(mel[:half][back], mel[half:])
    # one output at a time: the same bits as the corresponding half of the both-outputs call, grouped and plain
    flat_only, none = hip_ctx.stft2048_features(xd, 441, want_flat=True, want_mel=False, frame_center=fc, frame_lo=lo, frame_hi=hi)
    assert none is None and torch.equal(flat_only, flat)
    none, mel_only = hip_ctx.stft2048_features(xd, 441, want_flat=False, want_mel=True, frame_center=fc, frame_lo=lo, frame_hi=hi)
    assert none is None and torch.equal(mel_only, mel)
    flat, mel = hip_ctx.stft2048_features(xd, 512, want_flat=True, want_mel=True)
    assert torch.equal(hip_ctx.stft2048_features(xd, 512, want_flat=True, want_mel=False)[0], flat)
    assert torch.equal(hip_ctx.stft2048_features(xd, 512, want_flat=False, want_mel=True)[1], mel)


# ---------------------------------------------------------------------------------------------------------------------
# onset_strength
# ---------------------------------------------------------------------------------------------------------------------
def _check_onset(hip_ctx, groups, hop, agg):
    mel = np.concatenate(groups, axis=0)
    gs = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).tolist()
    env = hip_ctx.onset_strength(hip_ctx.to_device(mel), hop, agg, group_start=gs).cpu().numpy()
    ref = R.onset_from_mel(mel, hop, agg, gs)
    assert env.shape == ref.shape
    np.testing.assert_allclose(env, ref, err_msg=f"hop={hop} {agg} groups={gs[:8]}", **ONSET_TOL)
    pad = R.onset_pad(hop)
    for a, b in zip(gs[:-1], gs[1:]):
        assert not env[a: min(b, a + pad)].any()          # the left padding is exact zeros
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["mean", "median"])
@pytest.mark.parametrize("hop", ONSET_HOPS)
def test_onset_strength_synthetic_mel(hip_ctx, hop, agg):
    pool = _onset_pool(hop, seed=hop)
    assert max(float(g.max()) for kind, _, g in pool if kind == "quiet") < 1.0          # a negative dB maximum
    for kind, n, g in pool:                                                              # one group per launch
        env = _check_onset(hip_ctx, [g], hop, agg)
        if kind in ("zeros", "flat"):
            assert not env.any()
    for i in range(0, len(pool), 3):                                                     # two groups
        _check_onset(hip_ctx, [pool[i][2], pool[(i + 7) % len(pool)][2]], hop, agg)
    rng = np.random.default_rng(hop + 1)
    _check_onset(hip_ctx, [pool[i][2] for i in rng.integers(0, len(pool), 200)], hop, agg)      # 200 groups
    # the median's two middle ranks among 120 equal values: exactly that value
    rng = np.random.default_rng(7)
    g = _onset_group("ties", 12, rng)
    env = _check_onset(hip_ctx, [g], hop, "median")
    ref = R.onset_from_mel(g, hop, "median")
    assert np.count_nonzero(ref) >= 2 and np.array_equal(env == 0.0, ref == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1e-2, 1e-4])
def test_onset_strength_quiet_song_end_to_end(hip_ctx, scale):
    """stft2048_features -> onset_strength against librosa's onset_strength of the same samples; at 1e-4 the song's loudest mel
    bin is at about -54 dB, so the group maximum travels through the ordered-bits key as a negative float."""
    x = (signals.c2_song(20.0, seed=3) * np.float32(scale)).astype(np.float32)
    for hop, agg in [(2205, "mean"), (512, "median"), (512, "mean")]:
        _, mel = hip_ctx.stft2048_features(hip_ctx.to_device(x), hop, want_flat=False, want_mel=True)
        if scale == 1e-4:
            assert float(mel.max()) < 1.0
        env = hip_ctx.onset_strength(mel, hop, agg).cpu().numpy()
        ref = L.onset_strength(x, sr=SR, hop_length=hop, aggregate=np.mean if agg == "mean" else np.median)
        assert env.shape == ref.shape
        np.testing.assert_allclose(env, ref, **ONSET_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# tempogram_reduce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("win", TG_WINS)
def test_tempogram_reduce_edges(hip_ctx, win):
    logprior = _tg_logprior(win)
    for n in _tg_lengths(win):
        for kind in _tg_envelopes(1, 0):
            env, ref_mean, ref_arg, near = _tg_case(win, n, kind)
            assert near.sum() <= TG_MAX_LEFT_OUT * n
            envd = hip_ctx.to_device(env)
            mean, arg = hip_ctx.tempogram_reduce(envd, win, logprior)
            assert mean.shape == (win,) and arg.shape == (n,)
            np.testing.assert_allclose(mean.cpu().numpy(), ref_mean, err_msg=f"n={n} {kind}", **TG_TOL)
            arg = arg.cpu().numpy()
            assert np.array_equal(arg[~near], ref_arg[~near]), (n, kind)
            # a prior of -inf everywhere: every score is -inf and the pick is lag 0, like np.argmax; the mean does not see the prior
            mean2, arg2 = hip_ctx.tempogram_reduce(envd, win, np.full(win, -np.inf))
            assert torch.equal(mean2, mean) and not arg2.any().item(), (n, kind)
            mean3, none = hip_ctx.tempogram_reduce(envd, win, logprior, want_argmax=False)
            assert none is None and torch.equal(mean3, mean)


@pytest.mark.gpu
def test_tempogram_reduce_refuses_windows_outside_2_to_1024(hip_ctx):
    env = hip_ctx.to_device(np.ones(10, np.float32))
    for win in (1, 1025):
        with pytest.raises(_native.NativeError, match=r"invalid argument: win must be in \[2, 1024\]"):
            hip_ctx.tempogram_reduce(env, win, np.zeros(win))


# ---------------------------------------------------------------------------------------------------------------------
# yin_f0
# ---------------------------------------------------------------------------------------------------------------------
def _check_yin(hip_ctx, x, name, sr, fmin, fmax, frame_length, hop, threshold=0.1):
    lo, hi = R.yin_periods(sr, fmin, fmax, frame_length)
    f0, cmnd = hip_ctx.yin_f0(hip_ctx.to_device(x), sr, fmin, fmax, frame_length=frame_length, hop=hop, threshold=threshold, want_cmnd=True)
    cmnd = cmnd.cpu().numpy()
    tag = f"{name} n={len(x)} frame={frame_length} hop={hop} sr={sr}"
    assert f0.shape == (1 + len(x) // hop,) and cmnd.shape == (len(f0), hi - lo + 1), tag
    np.testing.assert_allclose(cmnd, R.cmnd_direct(x, sr, fmin, fmax, frame_length, hop), err_msg=tag, **CMND_TOL)
    period = sr / f0
    # the selection and the refinement, on the kernel's own series: no tie hazard, the same float64 formula on the same numbers
    np.testing.assert_allclose(period, R.yin_pick(cmnd, lo, threshold), rtol=1e-12, err_msg=tag)
    f0_nc, none = hip_ctx.yin_f0(hip_ctx.to_device(x), sr, fmin, fmax, frame_length=frame_length, hop=hop, threshold=threshold)
    assert none is None and np.array_equal(f0_nc, f0)
    return f0, lo, hi, cmnd


def _check_yin_shape(hip_ctx, sr, fmin, fmax, frame_length):
    """Every hop, length and signal of the issue's list at one frame length and lag range."""
    for hop in (128, 441, 512):
        for n in _yin_lengths(frame_length):
            for name, x in _yin_signals(n, sr, fmin, fmax, frame_length, seed=n + hop).items():
                f0, lo, hi, _ = _check_yin(hip_ctx, x, name, sr, fmin, fmax, frame_length, hop)
                if name == "silence":
                    assert np.all(f0 == sr / float(lo))            # cmnd == 0 everywhere: the first lag, no shift
                if n == 3 * frame_length + 17 and hop == 128:      # frames that lie wholly inside the tone
                    if name == "first_lag":
                        assert np.any(f0 == sr / float(lo))        # a pick at lag index 0: no parabolic shift
                    if name == "last_lag":
                        assert np.any(f0 == sr / float(hi))        # and at the last lag


def _check_yin_voiced(hip_ctx, sr, fmin, fmax, frame_length, hop):
    y = _yin_voiced(sr, fmin, fmax, frame_length)
    f0, _ = hip_ctx.yin_f0(hip_ctx.to_device(y), sr, fmin, fmax, frame_length=frame_length, hop=hop)
    ref_cm, _, _ = L.cmnd_frames(y, sr, fmin, fmax, frame_length, hop)
    strong = ref_cm.min(axis=0) < 0.05
    assert strong.sum() >= 20
    np.testing.assert_allclose(f0[strong], L.yin(y, fmin, fmax, sr=sr, frame_length=frame_length, hop_length=hop)[strong], rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(YIN_RANGES))
@pytest.mark.parametrize("frame_length", [64, 1024, 2048])
def test_yin_f0_edges(hip_ctx, frame_length, key):
    sr, fmin, fmax = YIN_RANGES[key]
    _check_yin_shape(hip_ctx, sr, fmin, fmax, frame_length)
    for hop in (128, 441, 512):
        _check_yin_voiced(hip_ctx, sr, fmin, fmax, frame_length, hop)


@pytest.mark.gpu
def test_yin_f0_trough_on_an_exact_plateau(hip_ctx):
    """A trough needs to be below its left neighbour and not above its right one: on these inputs the first trough EQUALS its right
    neighbour (cmnd exactly 1.0 twice, threshold 1.5), so `<=` and `<` on the right pick different lags."""
    q = YIN_PLATEAU
    for name, x in _yin_plateau_signals().items():
        f0, lo, hi, cmnd = _check_yin(hip_ctx, x, name, q["sr"], q["fmin"], q["fmax"], q["frame_length"], q["hop"], q["threshold"])
        assert _plateau_frames(cmnd, q["threshold"]), name             # on the kernel's own series


@pytest.mark.gpu
def test_yin_f0_frame_4096_needs_more_than_64_kib_of_lds(hip_ctx):
    """frame_length 4096 is the one admitted shape whose dynamic LDS passes 64 KiB: (2 * 4096 + 1 + 2 * (max_period + 1)) doubles,
    98 312 bytes at the largest max_period (2047) plus 96 bytes of static arrays, inside the 160 KiB (163 840 bytes) that a gfx950
    compute unit grants one workgroup; ac_yin_f0 raises the kernel's dynamic limit with hipFuncSetAttribute first.  The contract
    asserted here: the launch is accepted and computes what the float64 reference computes, over the same hops, lengths and signals
    as the smaller frames and at three lag ranges (max_period 2047, 675 and 320).  Kept last in the file."""
    frame_length = 4096
    for sr, fmin, fmax in [(44100, 20.0, 2093.004522404789), YIN_RANGES["music"], YIN_RANGES["speech_open"]]:
        lo, hi = R.yin_periods(sr, fmin, fmax, frame_length)
        assert (2 * frame_length + 1 + 2 * (hi + 1)) * 8 > 64 * 1024 and (2 * frame_length + 1 + 2 * (hi + 1)) * 8 + 96 <= 160 * 1024
        _check_yin_shape(hip_ctx, sr, fmin, fmax, frame_length)
    assert R.yin_periods(44100, 20.0, 2093.004522404789, frame_length)[1] == 2047
    for key in YIN_RANGES:
        for hop in (128, 441, 512):
            _check_yin_voiced(hip_ctx, *YIN_RANGES[key], frame_length, hop)
