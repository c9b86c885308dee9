"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files under the 64 MB cap, the same
files for the same result.  CPU only (a split_track-shaped result built by hand)."""
import dataclasses

import numpy as np
import pytest

import bench
from audio_cut_amd.analysis.features_cache import TrackFeatureCache
from audio_cut_amd.analysis.rhythm import BPMFeatures
from audio_cut_amd.cutting.refine import CutAdjustment
from audio_cut_amd.detectors.pure_vocal_pause_detector import PureVocalPause

SR = 44100


def _result(n: int) -> dict:
    rng = np.random.default_rng(7)
    cache = {f.name: None for f in dataclasses.fields(TrackFeatureCache)}
    cache.update(sr=SR, hop_length=2205, hop_s=0.05, duration_s=n / SR, rms_series=rng.random(n // 2205, dtype=np.float32),
                 spectral_flatness=rng.random(n // 2205), onset_envelope=rng.random(n // 2205), onset_strength=rng.random(n // 2205),
                 onset_frames=np.arange(4), rms_max=1.0, onset_max=2.0, bpm_features=BPMFeatures(120.0, "medium", 0.5, 0.9, 0.1),
                 tempo_curve=None, beat_times=np.arange(4) * 0.5, global_mdd=0.3, mdd_series=rng.random(n // 2205))
    # the vocal stem's samples are their own positions (float32 holds every integer below 2**24 exactly)
    return {"vocal_track": np.arange(n, dtype=np.float32), "instrumental_track": rng.standard_normal(n, dtype=np.float32),
            "sample_boundaries": [0, 44100, n], "refine_boundaries": [0, 44100, n], "cuts_samples": [0, 44100, n],
            "cuts_sec": [0.0, 1.0, n / SR], "segment_vocal_flags": [True, False], "segment_spans": [(0, 44100), (44100, n)],
            "cut_candidates": [(1.0, 0.5)], "num_pauses": 1, "separation_confidence": 0.9, "suppressed_cut_points_sec": [],
            "pauses": [PureVocalPause(0.9, 1.1, 0.2, "short", 0.5, {}, cut_point=1.0)],
            "guard_adjustments": [CutAdjustment(1.0, 1.0, 1.0, 0.5, 0.0, 0.0)], "vad_segments": [{"start": 0.5, "end": 2.0}],
            "guard_adjustments_unfiltered": [CutAdjustment(1.0, 1.0, 1.0, 0.5, 0.0, 0.0), CutAdjustment(3.0, 3.1, 3.1, 0.2, 100.0, 100.0)],
            "guard_shift_stats": {"avg_shift_ms": 0.0, "p95_shift_ms": 0.0, "count": 1}, "precision_guard_ok": True,
            "segment_layout_applied": False, "precision_guard_threshold_ms": {"avg": 15.0, "p95": 30.0}, "mode": "v2.2_mdd",
            "feature_cache": TrackFeatureCache(**cache), "timings": {"separate_s": 0.1}, "gpu_meta": {"x": 1}}


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_dump_outputs_float_files_under_the_cap_and_repeatable(tmp_path):
    res = _result(240 * SR)                                   # a full bench track: the stems alone would be 85 MB
    info = bench.dump_outputs(res, tmp_path / "a")
    bench.dump_outputs(res, tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert info["files"] == len(a) and sorted(a) == sorted(b)
    assert sum(v.nbytes for v in a.values()) == info["bytes"] <= bench.DUMP_LIMIT_BYTES
    assert all(v.dtype in (np.float32, np.float64) and v.size for v in a.values())
    assert "suppressed_cut_points_sec" not in a                 # empty in this result: no file
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert "timings" not in a and "gpu_meta" not in a
    assert a["sample_boundaries"].tolist() == [0, 44100, 240 * SR]
    assert a["pauses"].shape == (1, 5) and a["guard_adjustments"].shape == (1, 6) and a["segment_spans"].shape == (2, 2)
    assert a["guard_adjustments_unfiltered"].shape == (2, 6) and a["guard_shift_stats_count"].tolist() == [1.0]
    assert a["precision_guard_ok"].tolist() == [1.0] and a["segment_layout_applied"].tolist() == [0.0]
    assert not any(k.startswith("precision_guard_threshold") or k == "mode" for k in a)
    pos = a["vocal_track_sampled"]                           # the positions the sample was taken at
    assert pos.shape == (bench.DUMP_STEM_SAMPLES,) and "vocal_track" not in a
    assert pos[0] >= 0 and pos[-1] < 240 * SR and np.all(np.diff(pos) > 0)      # inside the stem, sorted, distinct
    assert np.array_equal(pos, pos.astype(np.int64)) and np.array_equal(a["instrumental_track_sampled"], res["instrumental_track"][pos.astype(np.int64)])


def test_dump_outputs_fails_on_a_non_numeric_output(tmp_path):
    res = _result(12 * SR)
    res["cuts_sec"] = [0.0, None, 12.0]
    with pytest.raises(TypeError, match="cuts_sec"):
        bench.dump_outputs(res, tmp_path)


def test_dump_outputs_short_stems_whole(tmp_path):
    res = _result(12 * SR)
    bench.dump_outputs(res, tmp_path)
    a = _load(tmp_path)
    assert np.array_equal(a["vocal_track"], res["vocal_track"]) and np.array_equal(a["instrumental_track"], res["instrumental_track"])
