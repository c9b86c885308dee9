"""Mode `vpbd_asr` on the GPU: `ac_resample_poly_pcm16` bit for bit against `ac_resample_poly` + the host's PCM_16 conversion and
within the float kernel's own bound of the oracle's resampler, `split_track(mode="vpbd_asr")` on seeded stems against the
reference's recorded results (tests/golden/vpbd_asr.json), and `separate_and_segment` end to end through the real separator."""
import json
import math
import types
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from audio_cut_amd import config as cfg
from audio_cut_amd.core.enhanced_vocal_separator import SeparationResult
from audio_cut_amd.lyrics import LyricsBoundaryCandidateGenerator, LyricsTimeline, attach_lyrics_to_segments
from audio_cut_amd.testing import signals
from audio_cut_amd.testing.lyrics_cases import asr_case, lyrics_case
from audio_cut_amd.testing.vpbd_inputs import FixedPauses
from audio_cut_amd.utils.audio_export import pcm_bytes_host

pytestmark = pytest.mark.gpu
SR = 44100
FIXTURE_KEY = "lyrics_alignment.fixture_path"


def _host_pcm16(x) -> np.ndarray:
    return pcm_bytes_host(np.asarray(x, dtype=np.float32), "PCM_16")[0].view("<i2")


def _noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


def _square(n):
    """full-scale square wave of period 74 behind 300 zeros: the resampler overshoots +-1 on most of it (Gibbs)."""
    x = np.zeros(n, dtype=np.float32)
    k = np.arange(max(0, n - 300))
    x[300:] = np.where((k // 37) % 2 == 0, 1.0, -1.0)
    return x


# ---- the kernel, exact ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 160, 441), (5, 160, 441), (300, 160, 441), (22, 160, 441), (13247, 160, 441), (4099, 147, 160), (1000, 3, 7)]


@pytest.mark.parametrize("n,up,down", SHAPES)
def test_pcm16_kernel_is_the_float_kernel_through_the_host_conversion(hip_ctx, n, up, down):
    n_out = -(-n * up // down)
    if (n, up) == (22, 160):
        assert n_out == 8
    if n == 13247:
        assert n_out == 4807 == 600 * 8 + 7
    for name, x in (("noise", _noise(n, n)), ("square", _square(n))):
        dev = hip_ctx.to_device(x)
        want = _host_pcm16(hip_ctx.resample_poly(dev, up, down).cpu().numpy())
        got = hip_ctx.resample_poly_pcm16(dev, up, down)
        assert got.dtype == np.int16 and got.shape == (n_out,)
        assert got.tobytes() == want.tobytes(), (name, int(np.count_nonzero(got != want)))
    if n == 13247:                                   # both saturation codes occur on the square wave
        got = hip_ctx.resample_poly_pcm16(hip_ctx.to_device(_square(n)), up, down)
        hi, lo = int(np.count_nonzero(got == 32767)), int(np.count_nonzero(got == -32768))
        print(f"square wave {n} -> {n_out}: {hi} samples at 0x7FFF, {lo} at 0x8000")
        assert hi > 100 and lo > 100


def test_pcm16_kernel_nan_padding_and_guard(hip_ctx):
    """One NaN input: the outputs whose taps touch it are 0, the others are untouched.  Called through the C ABI on a buffer
    with a guard: the last group's samples past n_out are zeros, and nothing is written behind the group."""
    n, up, down = 13247, 160, 441
    x = _noise(n, 7)
    x[6000] = np.nan
    dev = hip_ctx.to_device(x)
    flt = hip_ctx.resample_poly(dev, up, down).cpu().numpy()
    got = hip_ctx.resample_poly_pcm16(dev, up, down)
    touched = np.isnan(flt)
    assert 50 < int(touched.sum()) < 400 and np.all(got[touched] == 0)
    clean = x.copy(); clean[6000] = 0.0
    ref = hip_ctx.resample_poly_pcm16(hip_ctx.to_device(clean), up, down)
    assert np.array_equal(got[~touched], ref[~touched])

    from audio_cut_amd._native import _check, _ptr, _stream
    g = math.gcd(up, down)
    hd, n_pre = hip_ctx._resample_filter_dev(up // g, down // g)
    for n_in in (13247, 22, 5):
        xs = hip_ctx.to_device(_noise(n_in, 11))
        n_out = -(-n_in * up // down)
        padded = -(-n_out // 8) * 8
        buf = torch.full((2 * padded + 64,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
        assert buf.data_ptr() % 16 == 0
        _check(hip_ctx.lib.ac_resample_poly_pcm16(hip_ctx._h, _ptr(xs), n_in, up // g, down // g, _ptr(hd), hd.numel(), n_pre, _ptr(buf), n_out, _stream()))
        host = buf.cpu().numpy()
        body = host[: 2 * padded].view("<i2")
        assert np.array_equal(body[:n_out], hip_ctx.resample_poly_pcm16(xs, up, down))
        assert np.all(body[n_out:] == 0) and np.all(host[2 * padded:] == 0xA5), n_in
    # a misaligned output is refused, not written
    from audio_cut_amd._native import NativeError
    with pytest.raises(NativeError):
        _check(hip_ctx.lib.ac_resample_poly_pcm16(hip_ctx._h, _ptr(xs), 5, up // g, down // g, _ptr(hd), hd.numel(), n_pre, buf.data_ptr() + 2, 2, _stream()))
    # equal rates never reach the kernel
    assert np.array_equal(hip_ctx.resample_poly_pcm16(hip_ctx.to_device(x[:100]), 7, 7), _host_pcm16(x[:100]))


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------
def _oracle_bracket(x, up, down):
    """[pcm16(y - tol), pcm16(y + tol)], y the oracle's resampler and tol the bound the float kernel is held to
    (`test_resample_poly_kernel_vs_oracle`): pcm16 is monotone, so this is that bound carried through the quantiser."""
    from oracle import resample as ORS
    y = ORS.resample(x, up, down).astype(np.float64)
    tol = 2e-6 * max(1.0, float(np.max(np.abs(y))))
    return _host_pcm16((y - tol).astype(np.float32)), _host_pcm16((y + tol).astype(np.float32)), y


@pytest.mark.parametrize("n,up,down", [(13247, 160, 441), (4099, 147, 160), (1000, 3, 7), (300, 160, 441)])
def test_pcm16_kernel_within_the_oracle_bracket(hip_ctx, n, up, down):
    for name, x in (("noise", _noise(n, 100 + n)), ("square", _square(n))):
        lo, hi, y = _oracle_bracket(x, up, down)
        got = hip_ctx.resample_poly_pcm16(hip_ctx.to_device(x), up, down)
        assert got.shape == lo.shape
        width = hi.astype(np.int64) - lo.astype(np.int64)
        outside = int(np.count_nonzero((got < lo) | (got > hi)))
        print(f"{name} {n} x {up}/{down}: peak |y| {np.max(np.abs(y)):.3f}, bracket width max {int(width.max())}, "
              f"{int(np.count_nonzero(width))} two-valued of {len(width)}, outside {outside}")
        assert int(width.max()) <= 1
        assert outside == 0


# ---- the mode on seeded stems ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "vpbd_asr.json").read_text(encoding="utf-8"))


def _plain(obj):
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


class _SeededSeparator:
    """The separator's place taken by seeded stems resident on the device (the pattern of tests/test_hybrid_gpu.py)."""

    def __init__(self, hip, vocal, cache):
        self._primary_backend = types.SimpleNamespace(hip=hip)
        self.hip, self.vocal, self.cache = hip, vocal, cache

    def separate_for_detection(self, audio, gpu_context=None, audio_dev=None, separation_gate=None, unet_stream=None):
        hip, inst = self.hip, np.zeros_like(self.vocal)
        state = {"hip": hip, "mix": hip.to_device(np.asarray(audio, dtype=np.float32)), "vocal": hip.to_device(self.vocal),
                 "instrumental": hip.to_device(inst)}
        return SeparationResult(vocal_track=self.vocal, instrumental_track=inst, separation_confidence=1.0, backend_used="seeded",
                                processing_time=0.0, quality_metrics={}, feature_cache=self.cache, vad_segments=[],
                                gpu_meta={"gpu_pipeline_used": False}, device_state=state)


def _split(hip, overrides, payload, tmp_path, *, audio, vocal, cache, pauses, sr=SR, output_dir=""):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    ov = dict(overrides)
    path = tmp_path / "timeline.json"
    path.write_text(json.dumps(payload, ensure_ascii=False), encoding="utf-8")
    ov[FIXTURE_KEY] = str(path)
    splitter = SeamlessSplitter(sr, separator=_SeededSeparator(hip, vocal, cache))
    splitter.pure_vocal_detector = FixedPauses(pauses)
    seen = []
    real = hip.resample_poly_pcm16
    hip.resample_poly_pcm16 = lambda *a: (seen.append(a[1:]), real(*a))[1]
    saved = cfg.snapshot()
    cfg.set_runtime_config(ov)
    try:
        res = splitter.split_track(audio, mode="vpbd_asr", input_path=str(tmp_path / "song.wav"), output_dir=output_dir)
    finally:
        cfg.restore(saved)
        del hip.resample_poly_pcm16
    assert seen == [(16000, sr)]                       # one ASR copy per track, from the resident stem
    return res, splitter


def _same_detection(res, want, *, planner_exact):
    got = _plain({"boundary_detection": res["boundary_detection"], "lyrics_alignment": res["lyrics_alignment"]})
    assert got["lyrics_alignment"] == want["lyrics_alignment"]
    for key, value in want["boundary_detection"].items():
        if key == "planner" and not planner_exact:      # the fixture's is `detect`'s: split_track adds where the guards moved each cut
            for k, v in value.items():
                assert got["boundary_detection"]["planner"][k] == v, k
            continue
        assert got["boundary_detection"][key] == value, key
    assert res["lyrics_cut_protection_applied"] is False


def test_split_track_simple_song_scenario(hip_ctx, golden, tmp_path):
    """the reference's integration scenario 1: 8 s of silence, one pause, the reference's own timeline file."""
    case = golden["integration"]["simple"]
    audio = np.zeros(int(case["sample_rate"] * case["seconds"]), dtype=np.float32)
    res, _ = _split(hip_ctx, case["config"], case["timeline"], tmp_path, audio=audio, vocal=audio, cache=None,
                    pauses=[types.SimpleNamespace(**p) for p in case["pauses"]], output_dir=str(tmp_path / "out"))
    want = case["result"]
    _same_detection(res, want, planner_exact=True)
    assert [int(c) for c in res["cuts_samples"]] == want["cut_points_samples"]
    assert list(res["segment_vocal_flags"]) == want["segment_vocal_flags"] and res["segment_layout_applied"] == want["segment_layout_applied"]
    with wave.open(str(tmp_path / "out" / "song_vocal_for_asr.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 8 * 16000)
        assert not any(w.readframes(w.getnframes()))


def test_split_track_priority_scenario(hip_ctx, golden, tmp_path):
    """scenario 2 (a breath at a sentence end, a long pause, beat candidates), at its 16 kHz: the ASR copy is the stem itself."""
    case = golden["integration"]["priority"]
    sr = case["sample_rate"]
    audio = np.zeros(int(sr * case["seconds"]), dtype=np.float32)
    cache = types.SimpleNamespace(beat_times=np.arange(0.0, 8.001, 0.5, dtype=np.float32), rms_series=np.full(160, 0.8, dtype=np.float32),
                                  hop_s=0.05, duration_s=8.0, mdd_series=np.full(160, 0.5, dtype=np.float32))
    res, _ = _split(hip_ctx, case["config"], case["timeline"], tmp_path, audio=audio, vocal=audio, cache=cache,
                    pauses=[types.SimpleNamespace(**p) for p in case["pauses"]], sr=sr)
    _same_detection(res, case["result"], planner_exact=False)
    assert not list(tmp_path.glob("**/*_vocal_for_asr.wav"))             # no output_dir: the provider gets the samples only


@pytest.mark.parametrize("index", [1, 2])          # a unified pool with beats and breaths, and a legacy pool
def test_split_track_seeded_cases(hip_ctx, golden, tmp_path, index):
    case = golden["detect"][index]
    cache, pauses, vocal, payload = asr_case(case["seed"], breaths=case["breaths"])
    ov = dict(case["overrides"], **{"segment_layout.enable": False})        # the seeded cache is not a TrackFeatureCache
    res, _ = _split(hip_ctx, ov, payload, tmp_path, audio=vocal, vocal=vocal, cache=cache, pauses=pauses)
    _same_detection(res, case["result"], planner_exact=False)
    words = res["lyrics_alignment"]["timeline"]["words"]
    assert res["cuts_samples"][0] == 0 and res["cuts_samples"][-1] == len(vocal) and len(words) == res["lyrics_alignment"]["word_count"]


def test_layout_hook_reads_the_vocal_stems_rms(hip_ctx, tmp_path):
    """`segment_layout.enable`: the refiner's cache carries the VOCAL stem's RMS (frame max(2 hop, 0.1 s)) and the timeline's
    boundaries and words; the series is librosa's of the stem."""
    from oracle import librosa_ops
    _, pauses, vocal, payload = asr_case(41)
    mix = (vocal + 0.05 * _noise(len(vocal), 5)).astype(np.float32)
    ov = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", "vpbd.candidate_debug_json": False,
          "segment_layout.enable": True, "segment_layout.soft_min_s": 3.0, "segment_layout.soft_max_s": 8.0}
    calls = {}
    from audio_cut_amd.cutting import segment_layout_refiner as SLR
    real = SLR.refine_layout
    SLR.refine_layout = lambda *a, **k: (calls.update(k), real(*a, **k))[1]
    try:
        res, splitter = _split(hip_ctx, ov, payload, tmp_path, audio=mix, vocal=vocal, cache=None, pauses=pauses)
    finally:
        SLR.refine_layout = real
    cache = res["feature_cache"]
    frame = max(2 * cache.hop_length, int(round(cache.sr * 0.1)))
    ref = librosa_ops.rms(y=vocal, frame_length=frame, hop_length=cache.hop_length)[0]
    want_len = cache.frame_count()
    ref = np.pad(ref, (0, max(0, want_len - ref.size)), constant_values=float(ref[-1]))[:want_len]
    got = np.asarray(calls["features"].rms_series)          # the cache the layout refiner was handed
    err = float(np.max(np.abs(got - ref) / np.maximum(ref, 1e-6)))
    print(f"vocal layout rms: {got.size} frames of {frame} samples, worst relative error {err:.2e}")
    assert got.shape == ref.shape and err <= 1e-6
    assert calls["features"] is not cache and calls["features"].rms_max == float(np.max(got))
    assert not np.array_equal(cache.rms_series, got)                      # the track's own cache still follows the mix
    assert calls["asr_word_intervals"] == splitter._collect_lyrics_word_intervals(res["lyrics_alignment"]) and calls["asr_word_intervals"]
    assert calls["asr_boundary_times"] == splitter._collect_lyrics_boundary_times(res["lyrics_alignment"]) and calls["asr_boundary_times"]


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _write_wav16(path, x):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def test_separate_and_segment_vpbd_asr_end_to_end(hip_ctx, tmp_path, monkeypatch):
    from audio_cut_amd import api
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    captured, real_split = [], SeamlessSplitter.split_track
    monkeypatch.setattr(SeamlessSplitter, "split_track", lambda self, *a, **k: (captured.append(real_split(self, *a, **k)), captured[-1])[1])
    seconds = 14.0
    loaded = _write_wav16(tmp_path / "song.wav", signals.c2_song(seconds, seed=9))
    n = len(loaded)
    payload = lyrics_case(9, seconds)
    fixture = tmp_path / "lyrics.json"
    fixture.write_text(json.dumps(payload, ensure_ascii=False), encoding="utf-8")
    timeline = LyricsTimeline.from_dict(payload, strict=True)
    out_dir = tmp_path / "out"
    on = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", FIXTURE_KEY: str(fixture)}
    man = api.separate_and_segment(input_uri=str(tmp_path / "song.wav"), export_dir=str(out_dir), mode="vpbd_asr", export_manifest=True,
                                   runtime_overrides=on)
    res = api.last_result()
    assert man["success"] is True and man["version"] == "vpbd_asr"
    assert man["boundary_detection"]["actual_mode"] == "vpbd_asr" and man["lyrics_alignment"]["fallback_reason"] is None
    assert man["lyrics_alignment"]["word_count"] == len(timeline.words) > 0
    assert man["boundary_detection"]["candidate_counts"]["lyrics"] == len(LyricsBoundaryCandidateGenerator().generate(timeline)) > 0
    assert res["lyrics_cut_protection_applied"] is False

    asr = out_dir / "song_vocal_for_asr.wav"
    with wave.open(str(asr), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        frames = w.getnframes()
        got = np.frombuffer(w.readframes(frames), dtype="<i2")
    assert frames == math.ceil(n * 160 / 441)
    vocal = captured[0]["vocal_track"]                                     # the result's vocal stem, as the splitter returned it
    assert vocal.dtype == np.float32 and vocal.shape == (n,)
    lo, hi, y = _oracle_bracket(vocal, 160, 441)
    outside = int(np.count_nonzero((got < lo) | (got > hi)))
    print(f"ASR copy: {frames} frames, peak {np.max(np.abs(y)):.3f}, outside the oracle bracket {outside}")
    assert outside == 0

    disk = json.loads((out_dir / "SegmentManifest.json").read_text(encoding="utf-8"))
    assert disk["segments"] == _plain(man["segments"]) and disk["lyrics_alignment"] == _plain(man["lyrics_alignment"])
    assert any(s.get("lyrics") for s in disk["segments"]) and all("lyrics" in s for s in disk["segments"])
    bare = [{k: v for k, v in s.items() if k != "lyrics"} for s in disk["segments"]]
    assert _plain(attach_lyrics_to_segments(bare, LyricsTimeline.from_dict(disk["lyrics_alignment"]["timeline"]))) == disk["segments"]

    off_dir = tmp_path / "off"
    man = api.separate_and_segment(input_uri=str(tmp_path / "song.wav"), export_dir=str(off_dir), mode="vpbd_asr", export_manifest=True,
                                   runtime_overrides=dict(on, **{"lyrics_alignment.enabled": False}))
    assert man["boundary_detection"]["actual_mode"] == "vpbd_acoustic" and man["lyrics_alignment"]["fallback_reason"] == "lyrics_alignment_disabled"
    assert not list(off_dir.glob("**/*_vocal_for_asr.wav")) and all("lyrics" not in s for s in man["segments"])

    # the export directory reaches the detector for the ASR copy alone: no mode starts writing the candidate debug JSON there
    # (`vpbd.candidate_debug_json` is on by default), and `candidate_debug_path` stays None as before this mode existed
    def written(d):
        return sorted(str(f.relative_to(d)) for f in d.rglob("*") if f.is_file())

    def listed(d, result, *extra):
        return sorted([str(Path(f).resolve().relative_to(d.resolve())) for f in result["saved_files"]] + ["SegmentManifest.json", *extra])
    assert written(off_dir) == listed(off_dir, api.last_result())
    assert man["boundary_detection"]["candidate_debug_path"] is None
    ac_dir = tmp_path / "acoustic"
    ac = api.separate_and_segment(input_uri=str(tmp_path / "song.wav"), export_dir=str(ac_dir), mode="vpbd_acoustic", export_manifest=True)
    assert written(ac_dir) == listed(ac_dir, api.last_result())
    assert ac["boundary_detection"]["candidate_debug_path"] is None and "lyrics_cut_protection_applied" not in api.last_result()
    assert [f.replace("vpbd_acoustic", "vpbd_asr") for f in written(ac_dir)] == written(off_dir)      # the same files, the mode in two names
    assert ac["boundary_detection"]["selected"] == man["boundary_detection"]["selected"] and ac["cuts"] == man["cuts"]
    assert written(out_dir) == listed(out_dir, res, "song_vocal_for_asr.wav")
