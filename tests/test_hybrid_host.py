"""Host side of mode `hybrid_mdd`: both strategies, `deduplicate_and_convert_cuts`, the flag remap, the micro-merge and the
config against the reference's recorded results (tests/golden/hybrid_mdd.npz, the gate's answers taken from the fixture), and the
bad arguments the entry point of include/audiocut_hip_hybrid.h refuses.  CPU only."""
import ctypes as C
import json

import numpy as np
import pytest

from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd import config as cfg
from audio_cut_amd.cutting import hybrid_strategies as HS
from audio_cut_amd.testing import hybrid_cases

SR = hybrid_cases.SR
NAMES = [c["name"] for c in hybrid_cases.CASES]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "hybrid_mdd.npz")


def _cases(golden):
    return {c["name"]: c for c in json.loads(str(golden["cases"]))}


def _splitter():
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    sp = object.__new__(SeamlessSplitter)                      # the host rules need no device
    sp.sample_rate = SR
    return sp


def _context(golden, case):
    name = case["name"]
    g = lambda k: golden[f"{name}__{k}"]
    eff = case["effective_config"]
    hy = eff["hybrid_mdd"]
    tempo, bar_duration, thr = (float(v) for v in g("scalars"))
    gate = {int(c): bool(q) for c, q in zip(g("gate_centers"), g("gate_quiet"))}
    return HS.SegmentationContext(
        audio=np.empty(case["n_samples"], dtype=np.int8), sample_rate=SR, tempo=tempo, beat_times=g("beats"), bar_times=g("bar_times"),
        bar_duration=bar_duration, mdd_cut_points_samples=[int(c) for c in g("mdd_cuts")], energy_threshold=thr,
        bar_energies=[float(v) for v in g("bar_energies")], bar_spectral_centroids=[float(v) for v in g("bar_centroids")],
        bar_spectral_bandwidths=[float(v) for v in g("bar_bandwidths")], quiet_gate=gate,
        config={"density": hy["density"], "enable_beat_cuts": hy["enable_beat_cuts"], "bars_per_cut": hy["bars_per_cut"],
                "min_segment_s": eff["soft_min_s"], "energy_percentile": hy["energy_percentile"],
                "snap_to_pause_ms": hy["beat_detection"]["snap_to_pause_ms"], "snap_tolerance_ms": hy["snap_tolerance_ms"],
                "vad_protection": hy["vad_protection"], "chorus_force_snap": hy["chorus_force_snap"], "guard_db": eff["guard_db"],
                "guard_win_ms": eff["guard_win_ms"]})


@pytest.mark.parametrize("name", NAMES)
def test_strategy_matches_the_reference(golden, name):
    case = _cases(golden)[name]
    strategy = {"snap_to_beat": HS.SnapToBeatStrategy, "beat_only": HS.BeatOnlyStrategy}[case["strategy"]]()
    assert strategy.name == case["strategy"]
    res = strategy.generate_cut_points(_context(golden, case))
    assert res.cut_points_samples == [int(c) for c in golden[f"{name}__strategy_cuts"]]
    assert res.lib_flags == [bool(f) for f in golden[f"{name}__strategy_flags"]]
    want = case["strategy_metadata"]
    assert {k: res.metadata[k] for k in want} == want
    assert res.metadata["segment_durations"] == [(b - a) / float(SR) for a, b in zip(res.cut_points_samples[:-1], res.cut_points_samples[1:])]


@pytest.mark.parametrize("name", NAMES)
def test_remap_and_micro_merge_match_the_reference(golden, name):
    case = _cases(golden)[name]
    g = lambda k: golden[f"{name}__{k}"].tolist()
    sp = _splitter()
    if g("refined_cuts") != g("strategy_cuts") or len(g("strategy_cuts")) > 2:
        assert sp._remap_lib_flags_to_refined_cuts(g("strategy_cuts"), g("strategy_flags"), g("refined_cuts")) == g("refined_flags")
    cuts, flags = sp._hybrid_micro_merge(g("refined_cuts"), g("refined_flags"), case["effective_config"]["micro_merge_s"])
    assert cuts == g("final_cuts") and flags == g("final_lib_flags")
    assert sum(flags) == case["lib_segment_count"]
    spans, _ = sp._sample_level_spans(case["n_samples"], cuts, g("final_vocal_flags"))
    assert [hi - lo for lo, hi in spans] == g("span_lengths")


def test_remap_edges():
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter as S
    assert S._remap_lib_flags_to_refined_cuts([0, 10, 20], [True, False], [7]) == []
    assert S._remap_lib_flags_to_refined_cuts([0], [], [0, 5, 9]) == [False, False]
    # the end of the track is never `_lib`, neither as a refined end nor as the nearest raw end; a missing flag is False
    assert S._remap_lib_flags_to_refined_cuts([0, 10, 20, 30], [True, True, True], [0, 12, 19, 28, 30]) == [True, True, False, False]
    assert S._remap_lib_flags_to_refined_cuts([0, 10, 20, 30], [True], [0, 9, 21, 30]) == [True, False, False]


@pytest.mark.parametrize("name", NAMES)
def test_config_matches_the_reference(golden, name):
    case = _cases(golden)[name]
    saved = cfg.snapshot()
    cfg.set_runtime_config(dict(case["overrides"]))
    try:
        assert cfg.get_hybrid_mdd_config(case["density"]) == case["effective_config"]["hybrid_mdd"]
        assert float(cfg.get_config("quality_control.enforce_quiet_cut.guard_db", 2.5)) == case["effective_config"]["guard_db"]
        assert float(cfg.get_config("quality_control.enforce_quiet_cut.win_ms", 80)) == case["effective_config"]["guard_win_ms"]
        assert float(cfg.get_config("segment_layout", {}).get("soft_min_s", 2.0)) == case["effective_config"]["soft_min_s"]
    finally:
        cfg.restore(saved)


def test_config_fallbacks_and_environment(monkeypatch):
    base = cfg.get_hybrid_mdd_config()
    assert (base["density"], base["energy_percentile"], base["bars_per_cut"], base["snap_tolerance_ms"]) == ("medium", 60, 2, 200)
    odd = cfg.get_hybrid_mdd_config("dense")                                    # no such preset: the medium one, under its own name
    assert odd["density"] == "dense" and (odd["energy_percentile"], odd["bars_per_cut"]) == (60, 2)
    assert cfg.get_hybrid_mdd_config("low")["bars_per_cut"] == 4 and cfg.get_hybrid_mdd_config("high")["energy_percentile"] == 40
    monkeypatch.setenv("AUDIOCUT_HYBRID_DENSITY", "high")
    monkeypatch.setenv("AUDIOCUT_HYBRID_LIB_ALIGNMENT", "beat_only")
    monkeypatch.setenv("AUDIOCUT_SNAP_TOLERANCE_MS", "not a number")            # does not convert: ignored
    monkeypatch.setenv("AUDIOCUT_VAD_PROTECTION", "no")
    monkeypatch.setenv("AUDIOCUT_CHORUS_FORCE_SNAP", "1")
    env = cfg.get_hybrid_mdd_config()
    assert (env["density"], env["bars_per_cut"], env["lib_alignment"], env["snap_tolerance_ms"]) == ("high", 1, "beat_only", 200)
    assert env["vad_protection"] is False and env["chorus_force_snap"] is True
    assert cfg.get_hybrid_mdd_config("low")["density"] == "low"                 # the argument beats the environment


def test_deduplicate_and_convert_cuts():
    d = HS.deduplicate_and_convert_cuts
    assert d([], SR, 2 * SR) == ([0, 2 * SR], [False])
    assert d([(0.0, False)], 0, 5) == ([0, 5], []) and d([], SR, -1) == ([0, 0], [])
    cuts, flags = d([(0.0, False), (1.5, True), (1.5, False), (0.5, False), (2.0, False)], SR, 2 * SR)
    assert cuts == [0, SR // 2, 66150, 2 * SR] and flags == [False, True, False]          # the first of two equal times wins
    # two cuts that truncate to one sample: the flags are re-aligned by the 0.1 s rule
    a = 1.0
    cuts, flags = d([(0.0, False), (a, False), (a + 1e-9, True), (2.0, False)], SR, 2 * SR)
    assert cuts == [0, SR, 2 * SR] and flags == [True, False]
    # a time past the end is clamped onto it, and 0 / the end are added when missing
    cuts, flags = d([(0.7, True), (9.0, True)], SR, 2 * SR)
    assert cuts == [0, int(0.7 * SR), 2 * SR] and len(flags) == 2 and flags[0] is True


def test_gate_decisions_and_missing_answers():
    floor_db, point_db, quiet = HS.gate_decisions(np.array([1e-8] * 10 + [1e-2] * 30), np.array([1e-8, 1e-2, 0.0, 0.0]),
                                                  np.array([10, 10, 0, 10]), 1.5)
    rms = np.sqrt(np.array([1e-8] * 10 + [1e-2] * 30)) + 1e-12
    assert floor_db == float(20.0 * np.log10(np.percentile(rms, 5)))
    assert quiet.tolist() == [True, False, True, True] and point_db[3] == 20.0 * np.log10(1e-12)
    f0, _, q0 = HS.gate_decisions(np.zeros(0), np.zeros(2), np.zeros(2, dtype=np.int64), 1.5)      # an empty track: quiet everywhere
    assert f0 == -120.0 and q0.tolist() == [True, True]
    assert HS.gate_half_window(SR, 80.0) == 3528 and HS.gate_half_window(SR, 0.001) == 1 and HS.gate_center(0.5000113, SR) == 22050
    ctx = HS.SegmentationContext(audio=np.empty(4 * SR, np.int8), sample_rate=SR, tempo=120.0, beat_times=np.array([1.0, 1.5, 2.0]),
                                 bar_times=np.array([0.0, 2.0, 4.0]), bar_duration=2.0, mdd_cut_points_samples=[0, int(1.45 * SR), 4 * SR],
                                 energy_threshold=0.0, bar_energies=[1.0, 1.0], quiet_gate={},
                                 config={"min_segment_s": 1.0, "energy_percentile": 0})
    ctx.bar_energies = [1.0, 1.0, 1.0, 1.0]
    ctx.bar_times = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    with pytest.raises(KeyError):                                   # a beat nobody gated is an error, not a guess
        HS.SnapToBeatStrategy().generate_cut_points(ctx)


def test_mode_is_listed_and_fixture_covers_what_it_must(golden):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    assert "hybrid_mdd" in SeamlessSplitter.SUPPORTED_MODES
    cases = _cases(golden)
    assert list(cases) == NAMES
    for live in hybrid_cases.CASES:
        assert {k: cases[live["name"]][k] for k in live} == live                 # the fixture was generated from these very cases
    assert all(json.loads(str(golden["coverage"])).values())
    assert float(golden["min_margin_gate_db"]) >= 1e-3 and float(golden["min_margin_ratio_frames"]) >= 1.0
    for key in ("bar_rel", "score_abs", "cv_abs", "range_abs"):
        assert float(golden[f"min_margin_{key}"]) >= 1e-3


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_quiet_gate_rejects_bad_arguments(lib):
    """Every refusal comes back as AC_E_INVALID with a message, before anything is launched; the empty call is a no-op.  The context
    handle is never read by the checks, so a placeholder stands in for one here (no device on this machine)."""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    call = lib.ac_quiet_gate_meansq
    assert call(None, buf, 8, 4, buf, 1, buf, 2, buf, buf, None) == -1                 # no context
    for args, word in [((buf, 8, 0, buf, 1, buf, 2, buf, buf), "half_win"), ((buf, -1, 4, buf, 1, buf, 0, buf, buf), "n"),
                       ((buf, 8, 4, buf, 1, buf, 3, buf, buf), "n_blocks"), ((buf, 9, 4, buf, 1, buf, 2, buf, buf), "n_blocks"),
                       ((buf, 8, 4, buf, -1, buf, 2, buf, buf), "n_centers"), ((None, 8, 4, buf, 1, buf, 2, buf, buf), "null"),
                       ((buf, 8, 4, None, 1, buf, 2, buf, buf), "null"), ((buf, 8, 4, buf, 1, None, 2, buf, buf), "null")]:
        assert call(ctx, *args, None) == -1, args
        assert word in lib.ac_last_error().decode(), (args, lib.ac_last_error())
    assert call(ctx, None, 0, 4, None, 0, None, 0, None, None, None) == 0             # n == 0 and no centres: nothing to do
