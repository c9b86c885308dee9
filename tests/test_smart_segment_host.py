"""Mode `librosa_onset` without a GPU: the pure host rules of audio_cut_amd/cutting/smart_segment.py against the reference's
recorded results (tests/golden/librosa_onset.npz, written by tests/golden/make_onset_golden.py), the mode's configuration,
and the bad arguments the entry points of include/audiocut_hip_onset.h refuse."""
import json
from pathlib import Path

import numpy as np
import pytest

from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd import config as cfg
from audio_cut_amd.cutting import smart_segment as SS

ROOT = Path(__file__).resolve().parent.parent
SR = 44100
TYPE_NAME = {0: "verse", 1: "chorus", 2: "chorus_peak"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "librosa_onset.npz")


def _cases(golden):
    return json.loads(str(golden["cases"]))


def test_fixture_covers_the_cases_and_margins(golden):
    cases = {c["name"]: c for c in _cases(golden)}
    assert {"c2_60s_low", "c2_60s_medium", "c2_60s_high", "c2_60s_custom", "c2_60s_gaps", "c1_60s_fail", "c2_60s_no_separation",
            "c2_240s", "c2_3s_short"} <= set(cases)
    assert cases["c1_60s_fail"]["success"] is False
    for key in ("min_margin_frame_db", "min_margin_bar_rel", "min_margin_segment_rel"):
        assert float(golden[key]) >= 1e-3, key
    assert len(golden["c2_60s_gaps__silence_boundaries"]) >= 2
    assert list(golden["c2_60s_gaps__cuts"]) != list(golden["c2_60s_low__cuts"])
    assert set(golden["c2_60s_low__flags"].tolist()) == {True, False}
    for preset in ("low", "medium", "high"):
        assert list(golden["c2_60s_custom__cuts"]) != list(golden[f"c2_60s_{preset}__cuts"]), preset
    assert list(golden["c2_3s_short__cuts"]) == [0, cases["c2_3s_short"]["n_samples"]]
    assert set(json.loads(str(golden["versions"]))) == {"numpy", "scipy"}


def test_host_rules_reproduce_every_case_exactly(golden):
    for case in _cases(golden):
        if not case["success"]:
            continue
        name = case["name"]
        saved = cfg.snapshot()
        cfg.set_runtime_config(dict(case["overrides"]))
        try:
            lo = cfg.get_librosa_onset_config()
            soft_min = float(cfg.get_config("segment_layout.soft_min_s", 2.0))
        finally:
            cfg.restore(saved)
        assert soft_min == case["soft_min_s"] and lo["density"] == case["density"]
        bpm, bar_duration = (float(v) for v in golden[f"{name}__scalars"])
        assert bar_duration == 60.0 / bpm * lo["beat"]["time_signature"]
        energies = [float(e) for e in golden[f"{name}__bar_energies"]]
        types, thr_c, thr_p = SS.classify_bars(energies, lo["energy_analysis"]["chorus_percentile"],
                                               lo["energy_analysis"]["chorus_peak_percentile"])
        assert types == [TYPE_NAME[int(c)] for c in golden[f"{name}__bar_types"]], name
        assert thr_c <= thr_p
        n = int(case["n_samples"])
        duration = n / float(SR)
        bar_times = SS.bar_grid(duration, bar_duration)
        assert len(bar_times) - 1 == len(energies), name
        silences = [float(s) for s in golden[f"{name}__silence_boundaries"]]
        times = SS.plan_bar_cuts(bar_times, types, silences, SS.density_config(lo), duration, soft_min)
        assert SS.to_sample_points(times, SR, n) == [int(c) for c in golden[f"{name}__cuts"]], name


def test_bar_frame_ranges_are_the_reference_masks():
    rng = np.random.default_rng(0)
    for n_frames, bar in ((5168, 1.9969), (259, 2.0), (300, 0.0031), (10, 7.5)):
        times = SS.rms_frame_times(n_frames, SR, 512)
        duration = (n_frames - 1) * 512 / SR + rng.uniform(0, 0.01)
        bars = SS.bar_grid(duration, bar)
        lo, hi = SS.bar_frame_ranges(times, bars)
        assert len(lo) == len(bars) - 1
        for b in range(len(lo)):
            mask = (times >= bars[b]) & (times < bars[b + 1])
            assert np.array_equal(np.flatnonzero(mask), np.arange(lo[b], hi[b])), (n_frames, bar, b)


def test_silence_boundaries_quirks():
    times = SS.rms_frame_times(100, SR, 512)
    flags = np.zeros(100, dtype=bool)
    flags[10:40] = True            # 30 frames = 0.348 s: kept; the midpoint is taken between the FRAME TIMES of its first silent and next loud frame
    flags[50:60] = True            # 0.116 s: too short
    flags[80:] = True              # still open at the end of the track: dropped
    got = SS.silence_boundaries(flags, times, 100 * 512 / SR, 0.3)
    assert got == [float(times[10]) + (float(times[40]) - float(times[10])) / 2]
    assert SS.silence_boundaries(np.ones(100, dtype=bool), times, 2.0, 0.3) == []


def test_density_config_and_cut_plan_rules():
    low, high = {"verse_bars": 8, "chorus_bars": 4}, {"verse_bars": 2, "chorus_bars": 1}
    assert SS.density_config({"density": "low"}) == low
    assert SS.density_config({"density": "medium"}) == {"verse_bars": 4, "chorus_bars": 2}
    assert SS.density_config({"density": "high"}) == high
    assert SS.density_config({"density": "nonsense"}) == {"verse_bars": 4, "chorus_bars": 2}
    assert SS.density_config({"density": "low", "density_custom": {"enable": True, "verse_bars": 3}}) == {"verse_bars": 3, "chorus_bars": 2}
    bars = SS.bar_grid(20.0, 2.0)                                   # 0, 2, ..., 20
    types = ["verse"] * 5 + ["chorus"] * 5
    assert SS.plan_bar_cuts(bars, types, [], high, 20.0, 2.0) == [0.0, 4.0, 8.0, 12.0, 14.0, 16.0, 18.0, 20.0]
    # a silence at 5.5 s forces a cut at the next bar line (6 s) and is itself a cut; the 0.5 s piece between them is merged away
    assert SS.plan_bar_cuts(bars, types, [5.5], low, 20.0, 1.0) == [0.0, 5.5, 14.0, 20.0]
    # the short-segment merge always keeps the last point - here the bar line past the end of a 3 s track - and the sample points
    # of such a plan are the whole track
    assert SS.plan_bar_cuts(SS.bar_grid(3.0, 2.0), ["verse", "verse"], [], high, 3.0, 5.0) == [4.0]
    assert SS.to_sample_points([4.0], SR, 132300) == [0, 132300]
    assert SS.to_sample_points([0.0, 1.99999, 4.0], SR, 176400) == [0, 88199, 176400]      # int(88199.56): truncated, not rounded
    assert SS.label_segments(None, None, [0, 10, 20]) == [True, True]
    assert SS.label_segments([10 * 0.04, 10 * 0.0001], [10 * 1.0, 10 * 1.0], [0, 10, 20]) == [False, False]
    assert SS.label_segments([10 * 0.1, 10 * 0.0001], [10 * 1.0, 10 * 1.0], [0, 10, 20]) == [True, False]
    assert SS.label_segments([10 * 0.0002, 10 * 0.00005], None, [0, 10, 20]) == [True, False]


def test_config_defaults_are_the_reference_effective_values(golden, monkeypatch):
    for key in ("AUDIOCUT_DENSITY", "AUDIOCUT_LIBROSA_USE_VOCAL", "AUDIOCUT_SILENCE_THRESHOLD_DB", "AUDIOCUT_SILENCE_MIN_DURATION"):
        monkeypatch.delenv(key, raising=False)
    effective = json.loads(str(golden["effective_config"]))
    assert cfg.get_librosa_onset_config() == effective["librosa_onset"]
    assert effective["librosa_onset"]["density"] == "low"
    assert float(cfg.get_config("segment_layout.soft_min_s", 2.0)) == effective["segment_layout.soft_min_s"]
    monkeypatch.setenv("AUDIOCUT_DENSITY", "high")
    monkeypatch.setenv("AUDIOCUT_SILENCE_THRESHOLD_DB", "-35.5")
    monkeypatch.setenv("AUDIOCUT_SILENCE_MIN_DURATION", "not a number")     # does not convert: ignored
    monkeypatch.setenv("AUDIOCUT_LIBROSA_USE_VOCAL", "False")
    got = cfg.get_librosa_onset_config()
    assert got["density"] == "high" and got["silence"] == {"threshold_db": -35.5, "min_duration": 0.3}
    assert got["use_vocal_separation"] is False
    assert SS.density_config(got) == {"verse_bars": 2, "chorus_bars": 1}


def test_mode_is_supported_and_failure_builds_a_manifest(tmp_path):
    from audio_cut_amd.api import _build_manifest
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    assert "librosa_onset" in SeamlessSplitter.SUPPORTED_MODES
    src = tmp_path / "in.npy"
    np.save(src, np.zeros(8, dtype=np.float32))
    failed = {"success": False, "error": "float division by zero", "input_file": str(src), "mode": "librosa_onset"}
    man = _build_manifest(result=failed, input_path=src, export_dir=tmp_path, mode="librosa_onset", sample_rate=SR, channels=1, layout_cfg={})
    assert man["success"] is False and man["version"] == "librosa_onset" and man["segments"] == [] and "smart_segmentation" not in man


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_onset_entry_points_reject_bad_arguments(lib):
    # null pointers / zero sizes come back as AC_E_INVALID with a message, never as a launch or an exception
    import ctypes as C
    assert lib.ac_bar_energy_silence(None, None, 0, None, None, 0, -40.0, None, None, None) == -1
    assert b"invalid argument" in lib.ac_last_error()
    assert lib.ac_segment_pair_energy(None, None, None, 0, None, None, 0, None, None) == -1
    assert b"invalid argument" in lib.ac_last_error()
    # non-null pointers with zero sizes: refused on the sizes, nothing is dereferenced or launched
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.ac_bar_energy_silence(p, p, 0, p, p, 1, -40.0, p, p, None) == -1
    assert b"sizes must be positive" in lib.ac_last_error()
    assert lib.ac_bar_energy_silence(p, p, 4, p, p, 0, -40.0, p, p, None) == -1
    assert lib.ac_segment_pair_energy(p, p, p, 0, p, p, 1, p, None) == -1
    assert b"sizes must be positive" in lib.ac_last_error()
    assert lib.ac_segment_pair_energy(p, p, p, 4, p, p, 0, p, None) == -1
