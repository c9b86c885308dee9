"""Smart-cut intent and AutoProfile on the GPU: `ac_abs_peak_coverage` exactly against numpy and the reference's recorded
results (tests/golden/auto_profile.json), `split_track` with the smart-cut runtime on seeded stems against the reference's
`_apply_smart_cut_runtime`, and `separate_and_segment(segments=, alignment=)` end to end through the real separator."""
import json
import types
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from audio_cut_amd import _native
from audio_cut_amd import config as cfg
from audio_cut_amd.core.enhanced_vocal_separator import SeparationResult
from audio_cut_amd.core.seamless_splitter import SeamlessSplitter, host_vocal_coverage
from audio_cut_amd.testing import profile_cases as PC
from audio_cut_amd.testing import signals
from audio_cut_amd.testing.lyrics_cases import asr_case
from audio_cut_amd.testing.vpbd_inputs import FixedPauses

pytestmark = pytest.mark.gpu
SR = 44100
SAME = "same_as_marked"
FIXTURE_KEY = "lyrics_alignment.fixture_path"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "auto_profile.json").read_text(encoding="utf-8"))


def _plain(obj):
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


def _bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def _numpy_reference(x, rel=0.03, abs_floor=1e-5):
    """The reference's lines (`seamless_splitter.py:884-889`) with their intermediate values: numpy compares the float32 array with
    the Python float rounded to float32."""
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    thr = max(peak * rel, abs_floor)
    return peak, np.float32(thr), int(np.count_nonzero(np.abs(x) >= thr))


def _check_signal(hip, x, want=None, **kw):
    """Kernel == numpy (== the golden row) on peak bits, threshold bits, count and coverage; twice, and through a view offset by one
    element."""
    n = int(x.size)
    peak, thr, count = _numpy_reference(x, **kw)
    dev = hip.to_device(x)
    shifted = hip.to_device(np.concatenate([np.asarray([7.0], dtype=np.float32), x]))[1:]
    assert shifted.data_ptr() % 8 == 4 and shifted.is_contiguous()
    runs = [hip.vocal_coverage(dev, **kw), hip.vocal_coverage(dev, **kw), hip.vocal_coverage(shifted, **kw)]
    for got in runs:
        assert isinstance(got[0], float) and isinstance(got[1], np.float32) and isinstance(got[2], int)
        assert (_bits(got[0]), _bits(got[1]), got[2]) == (_bits(peak), _bits(thr), count), (n, got, (peak, thr, count))
    coverage = _native.coverage_from(runs[0][0], runs[0][2], n)
    if not kw:
        assert coverage == host_vocal_coverage(x)
    if want is not None:
        assert (_bits(peak), _bits(thr), count, coverage) == (want["peak_bits"], want["thr_bits"], want["count"], want["coverage"]), want
    return runs[0]


# ---- the kernel, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ("noise_half",) + PC.EDGE_RECIPES)
def test_coverage_kernel_exact(hip_ctx, golden, recipe):
    """Every case of the recipe: the small sizes sit around one wave (64), one workgroup row (256) and four tiles of 1024 (more than
    one workgroup); the largest `noise_half` case, 2 * PROFILE_GRID_SAMPLES + 5 samples, is past twice what one step of the capped
    grid (2048 workgroups x 1024 samples) covers, so every thread of both sweeps goes round its grid-stride loop at least twice
    and the last tile is partial."""
    rows = [r for r in golden["coverage"] if r["recipe"] == recipe]
    assert len(rows) >= 4
    if recipe == "noise_half":
        assert [r["n"] for r in rows] == list(PC.SMALL_SIZES) + [2 * _native.PROFILE_GRID_SAMPLES + 5]
    for want in rows:
        x = PC.coverage_signal(recipe, want["n"], want["seed"])
        peak, thr, count = _check_signal(hip_ctx, x, want)
        if recipe == "zeros":
            assert (peak, thr, count) == (0.0, np.float32(1e-5), 0) and want["coverage"] == 0.0
        if recipe == "peak_5e-10":
            assert peak == float(np.float32(5e-10)) and count == 0 and want["coverage"] == 0.0
        if recipe == "peak_2e-9":
            assert peak == float(np.float32(2e-9)) > 1e-9 and thr == np.float32(1e-5) and count == 0
        if recipe == "floor_edges" and want["n"] >= 65:
            assert peak == float(np.float32(1e-4)) and thr == np.float32(1e-5)
            at = np.float32(1e-5)
            below, above = np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(1))
            assert np.count_nonzero(np.abs(x) == at) >= 2 and np.count_nonzero(np.abs(x) == below) >= 2 and np.count_nonzero(x == above) >= 1
        if recipe == "thr_rounds_down" and want["n"] >= 65:
            assert float(thr) < peak * 0.03 and np.count_nonzero(np.abs(x) == thr) >= 2          # counted although below the float64 product
            assert count == int(np.count_nonzero(np.abs(x).astype(np.float64) >= float(thr))) > int(np.count_nonzero(np.abs(x).astype(np.float64) >= peak * 0.03))
        if recipe == "negative_peak":
            assert float(np.min(x)) == -peak and float(np.max(x)) < peak
        if recipe == "zeros_denormals":
            assert 0.0 < peak < 1.2e-38 or want["n"] == 1
            assert count == 0 and want["coverage"] == 0.0
        if recipe == "peak_last":
            assert x[-1] == np.float32(0.875) == np.float32(peak)
        if recipe == "peak_first":
            assert x[0] == np.float32(0.875) == np.float32(peak)


def test_coverage_kernel_empty_denormal_threshold_and_other_parameters(hip_ctx):
    empty = torch.empty(0, dtype=torch.float32, device=hip_ctx.device)
    assert hip_ctx.vocal_coverage(empty) == (0.0, np.float32(0.0), 0) and _native.coverage_from(0.0, 0, 0) == 0.0
    # no floor: the threshold of a denormal peak is a denormal, and denormals are compared as values, not flushed
    x = PC.coverage_signal("zeros_denormals", 4097, 3)
    peak, thr, count = _check_signal(hip_ctx, x, rel=0.5, abs_floor=0.0)
    assert 0.0 < float(thr) < 1.2e-38 and 0 < count < x.size
    # rel 0 and floor 0: everything counts, -0.0 included
    x = PC.coverage_signal("signal_with_denormals", 4095, 4)
    assert _check_signal(hip_ctx, x, rel=0.0, abs_floor=0.0)[2] == x.size
    assert _check_signal(hip_ctx, x, rel=1.0, abs_floor=0.0)[2] == int(np.count_nonzero(np.abs(x) == np.max(np.abs(x))))
    _check_signal(hip_ctx, PC.coverage_signal("noise_half", 70001, 5), rel=0.25, abs_floor=0.05)


def test_coverage_kernel_writes_its_outputs_only_and_refuses_bad_arguments(hip_ctx):
    from audio_cut_amd._native import NativeError, _check, _ptr, _stream
    lib, h = hip_ctx.lib, hip_ctx._h
    x = hip_ctx.to_device(PC.coverage_signal("noise_half", 4097, 6))
    buf = torch.full((6,), -1, dtype=torch.int64, device=hip_ctx.device)         # 16 bytes of outputs between two guards of 16
    base = buf.data_ptr() + 16
    _check(lib.ac_abs_peak_coverage(h, _ptr(x), 4097, 0.03, 1e-5, base, base + 4, base + 8, _stream()))
    host = buf.cpu().numpy()
    assert np.all(host[[0, 1, 4, 5]] == -1)
    want = hip_ctx.vocal_coverage(x)
    f = host[2:3].view(np.float32)
    assert (float(f[0]), np.float32(f[1]), int(host[3])) == want
    out = torch.zeros(2, dtype=torch.int64, device=hip_ctx.device)
    o = out.data_ptr()
    bad = [
        (None, _ptr(x), 16, 0.03, 1e-5, o, o + 4, o + 8),            # no context
        (h, _ptr(x), -1, 0.03, 1e-5, o, o + 4, o + 8),               # n < 0
        (h, _ptr(x), 1 << 40, 0.03, 1e-5, o, o + 4, o + 8),          # n >= 2^40
        (h, None, 16, 0.03, 1e-5, o, o + 4, o + 8),                  # no signal
        (h, _ptr(x), 16, 0.03, 1e-5, None, o + 4, o + 8),            # no outputs
        (h, _ptr(x), 16, 0.03, 1e-5, o, None, o + 8),
        (h, _ptr(x), 16, 0.03, 1e-5, o, o + 4, None),
        (h, _ptr(x), 16, -0.03, 1e-5, o, o + 4, o + 8),              # negative parameters
        (h, _ptr(x), 16, 0.03, -1e-5, o, o + 4, o + 8),
        (h, _ptr(x), 16, float("nan"), 1e-5, o, o + 4, o + 8),
    ]
    for args in bad:
        with pytest.raises(NativeError, match="invalid argument"):
            _check(lib.ac_abs_peak_coverage(*args, _stream()))
    torch.cuda.synchronize()
    assert torch.count_nonzero(out).item() == 0                        # a refused call launches nothing
    _check(lib.ac_abs_peak_coverage(h, None, 0, 0.03, 1e-5, base, base + 4, base + 8, _stream()))      # n == 0 needs no signal
    assert np.all(buf.cpu().numpy()[[2, 3]] == 0)
    with pytest.raises(NativeError):
        hip_ctx.vocal_coverage(x.double())


# ---- `split_track` on seeded stems -----------------------------------------------------------------------------------------------
class _SeededSeparator:
    """The separator's place taken by seeded stems resident on the device (the pattern of tests/test_vpbd_asr_gpu.py)."""

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


BASE = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", "vpbd.candidate_debug_json": False,
        "segment_layout.enable": False}                # the seeded cache is not a TrackFeatureCache


def _split(hip, spec, tmp_path, monkeypatch, *, mode, dotted, marked=True, watch=(), **kwargs):
    """-> (result, what the detector saw of the configuration, the coverage calls).  `dotted` goes in marked or unmarked, the
    rest of the run's configuration (provider, fixture) unmarked."""
    cache, pauses, vocal, payload = PC.smart_cut_case(spec)
    path = tmp_path / "timeline.json"
    path.write_text(json.dumps(payload, ensure_ascii=False), encoding="utf-8")
    splitter = SeamlessSplitter(SR, separator=_SeededSeparator(hip, vocal, cache))
    splitter.pure_vocal_detector = FixedPauses(pauses)
    seen, calls = {}, []
    real_detect = splitter.vpbd_detector.detect
    splitter.vpbd_detector.detect = lambda **k: (seen.update({key: _plain(cfg.get_config(key)) for key in watch}), real_detect(**k))[1]
    real_cov = _native.Context.vocal_coverage
    monkeypatch.setattr(_native.Context, "vocal_coverage", lambda self, x, *a, **k: (calls.append(x), real_cov(self, x, *a, **k))[1])
    saved = cfg.snapshot()
    cfg.set_runtime_config(dict(BASE, **{FIXTURE_KEY: str(path)}), explicit=False)
    cfg.set_runtime_config(dict(dotted), explicit=marked)
    before, marks = cfg.snapshot(), cfg.get_runtime_override_keys()
    try:
        res = splitter.split_track(vocal, mode=mode, input_path=str(tmp_path / "song.wav"), **kwargs)
        assert cfg.snapshot() == before and cfg.get_runtime_override_keys() == marks        # put back as it was found
    finally:
        cfg.restore(saved)
        monkeypatch.setattr(_native.Context, "vocal_coverage", real_cov)
    return res, seen, calls, cache


@pytest.mark.parametrize("seed,mode", [(41, "vpbd_asr"), (43, "vpbd_acoustic"), (45, "vpbd_acoustic"), (48, "vpbd_asr"), (49, "vpbd_acoustic"),
                                       (50, "vpbd_asr")])
def test_split_track_applies_the_smart_cut_runtime(hip_ctx, golden, tmp_path, monkeypatch, seed, mode):
    spec = next(s for s in PC.SMART_CUT_CASES if s["seed"] == seed)
    row = next(r for r in golden["runtime"]["seeded"] if r["seed"] == spec["seed"])
    for marked in (True, False):
        want = PC.expected_run(row, marked, golden["runtime"]["auto_applied_overrides"])
        watch = [k for k in want["config"] if k.startswith(("phrase_boundary.weights.", "vpbd.beat_candidates.", "global_planner.",
                                                                  "quality_control.", "pure_vocal_detection.", "segment_layout."))]
        res, seen, calls, cache = _split(hip_ctx, spec, tmp_path, monkeypatch, mode=mode, dotted=spec["smart_cut"], marked=marked, watch=watch)
        assert res["success"] and res["mode"] == mode
        assert _plain(res.get("auto_profile")) == want["meta"] and _plain(res["intent"]) == want["intent"]
        assert res["intent"]["applied_overrides"] == want["intent"]["applied_overrides"]
        assert seen == {k: want["config"][k] for k in watch} and len(seen) >= 7      # the detector ran on the overridden configuration
        stem = res["device_state"]["vocal"]
        if want["meta"] is None or spec.get("coverage") is not None:               # a named profile / a ratio already on the cache
            assert calls == []
        else:
            assert len(calls) == 1 and calls[0] is stem                             # one sweep, of the resident stem
            assert cache.vocal_coverage_ratio == want["coverage"] == host_vocal_coverage(res["vocal_track"])
        assert res["cuts_samples"][0] == 0 and res["cuts_samples"][-1] == len(res["vocal_track"])
        if mode == "vpbd_asr":
            assert res["lyrics_alignment"]["word_count"] > 0 and res["boundary_detection"]["actual_mode"] == "vpbd_asr"
    if row["unmarked"] != SAME:
        assert "config" in row["unmarked"]                                          # marking the keys changed what was written


def test_split_track_without_smart_cut_is_unchanged_and_flags_decide(hip_ctx, golden_dir, tmp_path, monkeypatch):
    """No `smart_cut.*` key and no flag: the result the mode gave before the smart-cut runtime existed (the reference's recorded
    detection, tests/golden/vpbd_asr.json), without the two blocks.  `smart_cut=False` with keys set is the same result;
    `smart_cut=True` without keys runs the runtime on the defaults; a gate refuses it."""
    asr_golden = json.loads((golden_dir / "vpbd_asr.json").read_text(encoding="utf-8"))
    case = asr_golden["detect"][1]
    spec = {"seed": case["seed"], "tempo": 120.0, "global_mdd": 0.5, "smart_cut": {}}
    monkeypatch.setattr(PC, "smart_cut_case", lambda s: asr_case(s["seed"], breaths=case["breaths"]))       # the cache as that golden saw it
    extra = {k: v for k, v in dict(case["overrides"], **{"segment_layout.enable": False}).items() if k != FIXTURE_KEY}
    plain, _, calls, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_asr", dotted=extra)
    assert "auto_profile" not in plain and "intent" not in plain and calls == []
    got = _plain({"boundary_detection": plain["boundary_detection"], "lyrics_alignment": plain["lyrics_alignment"]})
    assert got["lyrics_alignment"] == case["result"]["lyrics_alignment"]
    for key, value in case["result"]["boundary_detection"].items():
        if key == "planner":
            assert all(got["boundary_detection"]["planner"][k] == v for k, v in value.items())
        else:
            assert got["boundary_detection"][key] == value, key
    monkeypatch.undo()

    spec = PC.SMART_CUT_CASES[0]
    base, _, calls0, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_acoustic", dotted={})
    off, _, calls1, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_acoustic", dotted=spec["smart_cut"], smart_cut=False)
    on, _, calls2, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_acoustic", dotted={}, smart_cut=True)
    keyed, _, _, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_acoustic", dotted=spec["smart_cut"])
    assert calls0 == calls1 == [] and len(calls2) == 1
    shared = ("cuts_samples", "sample_boundaries", "segment_vocal_flags", "cut_candidates", "num_pauses", "vpbd_selected_times",
              "guard_shift_stats", "precision_guard_ok", "segment_layout_applied", "suppressed_cut_points_sec")
    for key in shared:
        assert _plain(base[key]) == _plain(off[key]), key
    assert _plain(base["boundary_detection"]) == _plain(off["boundary_detection"])
    assert all(k not in base and k not in off for k in ("auto_profile", "intent"))
    assert set(on) - set(base) == {"auto_profile", "intent"} and on["intent"]["segments"] == "medium" and on["intent"]["applied_overrides"] == []
    assert keyed["intent"]["segments"] == "many" and keyed["cuts_samples"] != base["cuts_samples"]       # the intent moves the cuts
    # a v2.2_mdd track ignores the keys, and refuses the flag
    mdd, _, calls3, _ = _split(hip_ctx, spec, tmp_path, monkeypatch, mode="v2.2_mdd", dotted=spec["smart_cut"])
    assert "intent" not in mdd and calls3 == []
    import threading
    for kwargs in ({"smart_cut": True, "separation_gate": threading.Lock()}, {"smart_cut": True, "unet_stream": torch.cuda.Stream()}):
        with pytest.raises(ValueError, match="one at a time"):
            _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_acoustic", dotted={}, **kwargs)
    with pytest.raises(ValueError, match="one at a time"):                        # keys in the configuration, with a gate
        _split(hip_ctx, spec, tmp_path, monkeypatch, mode="vpbd_asr", dotted=spec["smart_cut"], separation_gate=threading.Lock())
    with pytest.raises(ValueError, match="smart_cut=True"):
        _split(hip_ctx, spec, tmp_path, monkeypatch, mode="v2.2_mdd", dotted={}, smart_cut=True)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _write_wav16(path, x):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())


def _comparable(manifest, out_dir):
    """A manifest without what differs between two runs of the same job: timings (the device's load and memory gauges that the
    `gpu` block samples while the job runs are readings of the same kind), and the export directory in its paths."""
    text = json.dumps(manifest, ensure_ascii=False, default=str).replace(str(Path(out_dir).resolve().as_posix()), "<out>")
    man = json.loads(text)
    man.pop("timings_ms", None)
    man.pop("manifest_path", None)
    for key in [k for k in man.get("gpu", {}) if "smi_" in k or "_mem_" in k or "time" in k or k.endswith(("_s", "_ms"))]:
        man["gpu"].pop(key)
    return man


def test_separate_and_segment_with_intent_end_to_end(hip_ctx, golden, tmp_path, monkeypatch):
    from audio_cut_amd import api
    from audio_cut_amd.core.vocal_phrase_boundary_detector import VocalPhraseBoundaryDetector
    captured, real_split = [], SeamlessSplitter.split_track
    monkeypatch.setattr(SeamlessSplitter, "split_track", lambda self, *a, **k: (captured.append(real_split(self, *a, **k)), captured[-1])[1])
    planner_cfg, real_detect = [], VocalPhraseBoundaryDetector.detect
    monkeypatch.setattr(VocalPhraseBoundaryDetector, "detect",
                        lambda self, **k: (planner_cfg.append(cfg.get_config("global_planner")), real_detect(self, **k))[1])
    cov_calls, real_cov = [], _native.Context.vocal_coverage
    monkeypatch.setattr(_native.Context, "vocal_coverage", lambda self, x, *a, **k: (cov_calls.append(x), real_cov(self, x, *a, **k))[1])
    seconds = 14.0
    src = tmp_path / "song.wav"
    _write_wav16(src, signals.c2_song(seconds, seed=9))
    before_cfg = cfg.snapshot()

    first = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "a"), export_manifest=True)
    assert first["version"] == "v2.2_mdd" and "intent" not in first and "auto_profile" not in first

    man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "b"), segments="many", alignment="beat_lean",
                                   export_manifest=True)
    res = captured[-1]
    assert man["version"] == "vpbd_asr" and man["success"] is True
    echo = next(r["intent"] for r in golden["api"] if r["segments"] == "many" and r["alignment"] == "beat_lean")
    applied = man["intent"]["applied_overrides"]
    assert _plain({k: v for k, v in man["intent"].items() if k != "applied_overrides"}) == echo
    assert applied == sorted(applied) and "vpbd.beat_candidates.base_score" in applied and "global_planner.beat_conflict_weight" in applied
    assert len([k for k in applied if k.startswith("phrase_boundary.weights.")]) == 8
    vocal = res["vocal_track"]
    auto = man["auto_profile"]
    assert auto["features"]["vocal_coverage_ratio"] == round(host_vocal_coverage(vocal), 4)
    assert len(cov_calls) == 1 and cov_calls[0] is res["device_state"]["vocal"]
    assert auto["alignment"] == {"value": 0.75, "raw": "beat_lean"} and auto["style"] in ("ballad", "pop", "rap", "edm")
    lyr = man["lyrics_alignment"]
    assert lyr["enabled"] is True and lyr["provider"] == "null" and lyr["fallback_reason"] == "lyrics_alignment_unavailable"
    assert man["boundary_detection"]["actual_mode"] == "vpbd_acoustic" and lyr["word_count"] == 0
    # the planner worked inside the hard limits of `many`: (3, 8) s -> 1.2 s .. 12 s
    assert (planner_cfg[-1]["hard_min_s"], planner_cfg[-1]["hard_max_s"], planner_cfg[-1]["target_min_s"], planner_cfg[-1]["target_max_s"]) == (1.2, 12.0, 3.0, 8.0)
    picked = [float(c["t"]) for c in man["boundary_detection"]["selected"]]
    if man["boundary_detection"]["planner"].get("planner") == "dynamic_programming":
        gaps = np.diff([0.0, *picked, len(vocal) / SR])
        print(f"many / beat_lean: {len(picked)} planned cuts, gaps {gaps.min():.2f} .. {gaps.max():.2f} s, style {auto['style']}")
        assert len(picked) >= 1 and gaps.min() >= 1.2 and gaps.max() <= 12.0
    disk = json.loads((tmp_path / "b" / "SegmentManifest.json").read_text(encoding="utf-8"))
    assert disk["intent"] == _plain(man["intent"]) and disk["auto_profile"] == _plain(man["auto_profile"])
    assert cfg.snapshot() == before_cfg and cfg.get_runtime_override_keys() == set()

    again = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "c"), export_manifest=True)
    assert "intent" not in again and "auto_profile" not in again and len(cov_calls) == 1
    assert _comparable(again, tmp_path / "c") == _comparable(first, tmp_path / "a")
