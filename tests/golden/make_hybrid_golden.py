#!/usr/bin/env python3
"""Generate tests/golden/hybrid_mdd.npz by running the reference's own `_process_hybrid_mdd_split`
(`src/vocal_smart_splitter/core/seamless_splitter.py:1351-1704`) - its `BeatAnalyzer`, both strategies,
`_finalize_and_filter_cuts_v2`, `_remap_lib_flags_to_refined_cuts`, `_classify_segments_vocal_presence`, the micro-merge and
`_split_at_sample_level` - over the oracle's librosa restatement.

Runs ONLY where the reference exists (/root/reference); the GPU box never sees it.  As in make_onset_golden.py,
`oracle.librosa_ops` is registered under the name `librosa` and the splitter is built with `object.__new__`: the track loader
returns the seeded mix, the separator the seeded stems and a feature cache holding the case's beats, `_process_pure_vocal_split`
the case's listed MDD cut samples, the exporter writes nothing and `build_base` returns its keyword arguments.

What the result does not carry is observed, not restated: the strategy's output, the guarded boundaries, the remapped flags and
the flags before the micro-merge are what the method's own calls returned, and every question the strategies asked
`is_quiet_vocal_window` is recorded with the `point_db` and `floor_db` of the reference's own `_rms_db` / `_vocal_floor_db`.

The fixture holds data only - seeds, parameters, effective config and recorded results - never a track or a stem.  Before
anything is written every decision taken on a float series must clear its threshold:
  * every gate decision: |point_db - (floor_db + guard_db)| >= 1e-3 dB;
  * the bar-energy and fused-score margins of make_beat_golden.py (1e-3, cv and ranges included);
  * every segment's vocal-activity ratio at least one frame away from its threshold.
A case that misses a margin gets another seed, never a smaller margin.  The coverage the case set must reach is asserted too.
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_beat_golden as MB  # noqa: E402  (registers the librosa stand-in with spectral_bandwidth, sets the paths)

from audio_cut_amd.testing import hybrid_cases  # noqa: E402
from vocal_smart_splitter.core import seamless_splitter as ref_ss  # noqa: E402
from vocal_smart_splitter.core.strategies import base as ref_base  # noqa: E402
from vocal_smart_splitter.core.strategies import beat_only_strategy as ref_bo  # noqa: E402
from vocal_smart_splitter.core.strategies import snap_to_beat_strategy as ref_snap  # noqa: E402
from vocal_smart_splitter.core.utils.result_builder import ResultBuilder  # noqa: E402
from vocal_smart_splitter.utils import config_manager as ref_cfg  # noqa: E402

SR = hybrid_cases.SR
MARGIN = 1e-3


def run_reference(case, mono, vocal, inst, beats):
    """-> (result dict, observations)."""
    n = len(mono)
    obs = {"gate": {}, "classify": [], "non_nearest": 0}
    fake = object.__new__(ref_ss.SeamlessSplitter)
    fake.sample_rate = SR
    fake._export_format = "wav"
    fake._export_options = {}
    fake._precision_guard_ok = True
    fake._last_segment_classification_debug = []
    fake._last_guard_shift_stats = fake._blank_guard_stats()
    fake._last_guard_adjustments = []
    fake._last_guard_adjustments_raw = []
    fake._last_suppressed_cut_points = []
    fake._load_and_resample_if_needed = lambda path: mono
    cache = types.SimpleNamespace(beat_times=np.asarray(beats, dtype=np.float64), bpm_features=None)
    fake.separator = types.SimpleNamespace(separate_for_detection=lambda audio: types.SimpleNamespace(
        vocal_track=vocal, instrumental_track=inst, feature_cache=cache, backend_used="seeded", separation_confidence=1.0, gpu_meta={}))
    mdd = hybrid_cases.mdd_cut_samples(case, n)
    fake._process_pure_vocal_split = lambda *a, **k: ({"success": True, "cut_points_samples": list(mdd)} if case["mdd_success"]
                                                       else {"success": False, "error": "stand-in MDD failure"})
    fake.beat_analyzer = ref_ss.BeatAnalyzer(sample_rate=SR)
    strategies = {"beat_only": ref_bo.BeatOnlyStrategy(), "snap_to_beat": ref_snap.SnapToBeatStrategy()}
    fake._hybrid_strategies = strategies
    fake.segment_exporter = types.SimpleNamespace(export_segments=lambda *a, **k: [], export_full_track=lambda *a, **k: "")
    real_rb = ResultBuilder(precision_guard_avg_ms=ref_ss.PRECISION_GUARD_AVG_MS, precision_guard_p95_ms=ref_ss.PRECISION_GUARD_P95_MS)
    fake.result_builder = types.SimpleNamespace(build_base=lambda **k: dict(k), add_hybrid_metadata=real_rb.add_hybrid_metadata,
                                                add_separation_metadata=lambda r, s: r)

    floor_cache = {}

    def gate_tap(audio, sample_rate, time, *, guard_win_ms, guard_db):
        quiet = ref_base.is_quiet_vocal_window(audio, sample_rate, time, guard_win_ms=guard_win_ms, guard_db=guard_db)
        center = int(round(time * sample_rate))
        half_win = max(1, int(round(sample_rate * guard_win_ms / 1000.0)))
        start, end = max(0, center - half_win), min(len(audio), center + half_win)
        if half_win not in floor_cache:
            floor_cache[half_win] = ref_base._vocal_floor_db(audio, half_win)
        point_db = ref_base._rms_db(audio[start:end]) if start < end else float("nan")
        assert audio is vocal
        obs["gate"][float(time)] = (center, point_db, floor_cache[half_win], bool(quiet), float(guard_db), half_win, end - start)
        return quiet

    for name, strat in strategies.items():
        real = strat.generate_cut_points

        def tap(context, _real=real, _name=name):
            res = _real(context)
            obs["strategy"] = (_name, list(res.cut_points_samples), list(res.lib_flags), res.metadata, context)
            return res
        strat.generate_cut_points = tap
    snap = strategies["snap_to_beat"]
    real_quiet_beat = snap._find_quiet_beat_within_tolerance

    def quiet_beat_tap(time, beat_times, *a, **k):
        got = real_quiet_beat(time, beat_times, *a, **k)
        if got is not None and got != snap._find_nearest_beat(time, beat_times):
            obs["non_nearest"] += 1
        return got
    snap._find_quiet_beat_within_tolerance = quiet_beat_tap

    real_fin = ref_ss.SeamlessSplitter._finalize_and_filter_cuts_v2

    def fin_tap(cands, audio, pure_vocal_audio=None):
        res = real_fin(fake, cands, audio, pure_vocal_audio=pure_vocal_audio)
        obs["refined"] = [int(b) for b in res.sample_boundaries]
        return res
    fake._finalize_and_filter_cuts_v2 = fin_tap
    real_remap = ref_ss.SeamlessSplitter._remap_lib_flags_to_refined_cuts

    def remap_tap(*a):
        obs["remapped"] = list(real_remap(*a))
        return list(obs["remapped"])
    fake._remap_lib_flags_to_refined_cuts = remap_tap
    real_cls = ref_ss.SeamlessSplitter._classify_segments_vocal_presence

    def cls_tap(vocal_audio, cut_points, **k):
        flags = real_cls(fake, vocal_audio, cut_points, **k)
        obs["classify"].append(([int(c) for c in cut_points], list(flags), [dict(d) for d in fake._last_segment_classification_debug]))
        return flags
    fake._classify_segments_vocal_presence = cls_tap
    real_split = ref_ss.SeamlessSplitter._split_at_sample_level

    def split_tap(audio, cuts, **k):
        out = real_split(fake, audio, cuts, **k)
        if "segment_flags" in k:
            obs["spans_len"] = [len(s) for s in out[0]]
        return out
    fake._split_at_sample_level = split_tap

    ref_snap.is_quiet_vocal_window, ref_bo.is_quiet_vocal_window = gate_tap, gate_tap
    try:
        res = fake._process_hybrid_mdd_split("track.wav", "/nonexistent", export_plan=("mix_segments",),
                                             density_override=case["density"])
    finally:
        ref_snap.is_quiet_vocal_window = ref_bo.is_quiet_vocal_window = ref_base.is_quiet_vocal_window
    obs["beat_result"] = fake.beat_analyzer.last_result if hasattr(fake.beat_analyzer, "last_result") else None
    obs["mdd"] = mdd
    return res, obs


def evaluate(case):
    name = case["name"]
    mix, vocal, inst, beats = hybrid_cases.build(case)
    mono = hybrid_cases.mono_of(mix)
    n = len(mono)
    ref_cfg.reset_runtime_config()
    ref_cfg.set_runtime_config(dict(case["overrides"]))
    try:
        hybrid_config = ref_cfg.get_hybrid_mdd_config(case["density"])
        guard_db = float(ref_cfg.get_config("quality_control.enforce_quiet_cut.guard_db", 2.5))
        guard_win_ms = float(ref_cfg.get_config("quality_control.enforce_quiet_cut.win_ms", 80))
        layout = dict(ref_cfg.get_config("segment_layout", {}) or {})
        ratio_thr = float(ref_cfg.get_config("quality_control.segment_vocal_activity_ratio", 0.10))
        res, obs = run_reference(case, mono, vocal, inst, beats)
    finally:
        ref_cfg.reset_runtime_config()
    strat_name, s_cuts, s_flags, s_meta, ctx = obs["strategy"]

    # margins: gate
    m_gate = np.inf
    for t, (center, point_db, floor_db, quiet, gdb, half_win, count) in obs["gate"].items():
        assert count > 0 and gdb == guard_db
        m_gate = min(m_gate, abs(point_db - (floor_db + gdb)))
        assert quiet == (point_db <= floor_db + gdb)
    # margins: bar energies and fused scores, as make_beat_golden.py takes them (the strategy's own percentile)
    e = np.asarray(ctx.bar_energies, dtype=np.float64)
    m_bar = m_score = m_cv = m_rng = np.inf
    chorus = set()
    if e.size:
        thr = float(np.percentile(ctx.bar_energies, float(hybrid_config["energy_percentile"])))
        off = e[e != thr]
        m_bar = float(np.min(np.abs(off - thr) / thr)) if off.size else np.inf
        chorus, scores, f_thr, cv = MB.run_fusion(ctx.bar_energies, thr, ctx.bar_spectral_centroids, ctx.bar_spectral_bandwidths)
        s64 = scores.astype(np.float64)
        off_s = s64[s64 != f_thr]
        m_score = float(np.min(np.abs(off_s - f_thr))) if off_s.size else np.inf
        m_cv = min(abs(cv - 0.15), abs(cv - 0.4))
        m_rng = min(MB._range_margin(v) for v in (ctx.bar_energies, ctx.bar_spectral_centroids, ctx.bar_spectral_bandwidths))
    # margins: vocal-activity ratio, in frames
    hop = max(1, int(0.02 * SR))
    frame_length = max(hop * 2, int(0.05 * SR))
    m_ratio = np.inf
    for cuts, flags, debug in obs["classify"]:
        for (a, b), d in zip(zip(cuts[:-1], cuts[1:]), debug):
            size = b - a
            if size >= frame_length:
                n_frames = 1 + size // hop
                m_ratio = min(m_ratio, abs(float(d["vocal_activity_ratio"]) - ratio_thr) * n_frames)
    print(f"  {name} (seed {case['seed']}): {strat_name} margins  gate {m_gate:.3e} dB  bar {m_bar:.3e}  score {m_score:.3e}  cv {m_cv:.3e}  "
          f"range {m_rng:.3e}  ratio {m_ratio:.2f} frames   chorus {sorted(chorus)}")
    assert m_gate >= MARGIN, (name, "gate margin", m_gate)
    assert m_bar >= MARGIN and m_score >= MARGIN and m_cv >= MARGIN and m_rng >= MARGIN, (name, m_bar, m_score, m_cv, m_rng)
    assert m_ratio >= 1.0, (name, "vocal-activity ratio margin (frames)", m_ratio)

    final_cuts = [int(c) for c in res["cut_points_samples"]]
    refined = obs.get("refined", list(s_cuts))
    refined = refined if len(refined) >= 2 else list(s_cuts)
    refined_flags = obs["remapped"] if ("remapped" in obs and refined is not s_cuts) else list(s_flags)
    merged_flags = [bool(f) for f in res["segment_lib_flags"]]
    spans_len = obs["spans_len"]
    gate_rows = sorted(obs["gate"].items())
    print(f"    mdd {obs['mdd']}\n    strategy cuts {s_cuts}\n    flags {s_flags}\n    refined {refined}\n    flags {refined_flags}\n"
          f"    final {final_cuts}\n    lib {merged_flags}  vocal {list(res['segment_vocal_flags'])}\n"
          f"    meta {s_meta.get('snap_stats', s_meta.get('vad_blocked'))}  gated {len(gate_rows)}")
    arrays = {
        "beats": np.asarray(beats, dtype=np.float64), "bar_times": np.asarray(ctx.bar_times, dtype=np.float64),
        "scalars": np.array([ctx.tempo, ctx.bar_duration, ctx.energy_threshold], dtype=np.float64),
        "bar_energies": e, "bar_centroids": np.asarray(ctx.bar_spectral_centroids, dtype=np.float64),
        "bar_bandwidths": np.asarray(ctx.bar_spectral_bandwidths, dtype=np.float64),
        "chorus_bars": np.asarray(sorted(chorus), dtype=np.int64),
        "gate_times": np.array([t for t, _ in gate_rows], dtype=np.float64),
        "gate_centers": np.array([v[0] for _, v in gate_rows], dtype=np.int64),
        "gate_point_db": np.array([v[1] for _, v in gate_rows], dtype=np.float64),
        "gate_floor_db": np.array([v[2] for _, v in gate_rows], dtype=np.float64),
        "gate_quiet": np.array([v[3] for _, v in gate_rows], dtype=bool),
        "mdd_cuts": np.asarray(obs["mdd"] if case["mdd_success"] else [], dtype=np.int64),
        "strategy_cuts": np.asarray(s_cuts, dtype=np.int64), "strategy_flags": np.asarray(s_flags, dtype=bool),
        "refined_cuts": np.asarray(refined, dtype=np.int64), "refined_flags": np.asarray(refined_flags, dtype=bool),
        "final_cuts": np.asarray(final_cuts, dtype=np.int64), "final_lib_flags": np.asarray(merged_flags, dtype=bool),
        "final_vocal_flags": np.asarray(list(res["segment_vocal_flags"]), dtype=bool),
        "span_lengths": np.asarray(spans_len, dtype=np.int64),
        "segment_durations": np.asarray(res["segment_durations"], dtype=np.float64),
    }
    meta = {"strategy": res["strategy"], "method": res["method"], "hybrid_config": res["hybrid_config"],
            "beat_analysis": res["beat_analysis"], "lib_segment_count": res["lib_segment_count"],
            "strategy_metadata": ({"snap_stats": s_meta["snap_stats"]} if strat_name == "snap_to_beat" else {"vad_blocked": s_meta["vad_blocked"]}),
            "effective_config": {"hybrid_mdd": hybrid_config, "guard_db": guard_db, "guard_win_ms": guard_win_ms,
                                 "soft_min_s": float(layout.get("soft_min_s", 2.0)), "micro_merge_s": float(layout.get("micro_merge_s", 2.0)),
                                 "segment_vocal_activity_ratio": ratio_thr},
            "n_samples": n}
    micro = meta["effective_config"]["micro_merge_s"]
    n_mdd_inside = len([c for c in obs["mdd"][1:-1]]) if case["mdd_success"] else 0
    bar_samples = {int(float(t) * SR) for t in ctx.bar_times}
    mdd_samples = set(obs["mdd"][1:-1])
    s_set = set(s_cuts)
    facts = {
        "strategy": strat_name, "density": hybrid_config["density"], "stats": s_meta.get("snap_stats"), "vad_blocked": s_meta.get("vad_blocked"),
        "non_nearest": obs["non_nearest"], "n_strategy_inside": len(s_cuts) - 2, "n_mdd_inside": n_mdd_inside,
        "moved_lib": any(refined_flags[i] and refined[i + 1] not in s_set for i in range(len(refined_flags))),
        "merge_drops_flag": len(final_cuts) < len(refined) and sum(merged_flags) < sum(refined_flags),
        "short_lib_survives": any(f and (b - a) / SR < micro for f, a, b in zip(merged_flags, final_cuts[:-1], final_cuts[1:])),
        "bo_mdd_verse": strat_name == "beat_only" and any((not f) and c in mdd_samples for f, c in zip(s_flags, s_cuts[1:])),
        "bo_fallback": strat_name == "beat_only" and any((not f) and c in bar_samples and c not in mdd_samples
                                                          for f, c in zip(s_flags[:-1], s_cuts[1:-1])),
        "lib_bar_start": strat_name == "snap_to_beat" and any(f and c in bar_samples for f, c in zip(s_flags, s_cuts[1:])),
        "force": bool(hybrid_config["chorus_force_snap"]), "unprotected": not hybrid_config["vad_protection"],
        "mdd_failed": not case["mdd_success"], "configured_alignment": hybrid_config["lib_alignment"],
        "few_beats": len(beats) < 2, "stereo": mix.ndim == 2,
    }
    margins = {"gate_db": m_gate, "bar_rel": m_bar, "score_abs": m_score, "cv_abs": m_cv, "range_abs": m_rng, "ratio_frames": m_ratio}
    return arrays, meta, margins, facts


def main() -> None:
    out, listing, facts = {}, [], {}
    mins = {}
    for case in hybrid_cases.CASES:
        arrays, meta, margins, f = evaluate(case)
        facts[case["name"]] = f
        for k, v in margins.items():
            mins[k] = min(mins.get(k, np.inf), v)
        listing.append(dict(case, **meta))
        for k, v in arrays.items():
            out[f"{case['name']}__{k}"] = v
    fs = list(facts.values())
    snaps = [f for f in fs if f["strategy"] == "snap_to_beat"]
    cover = {
        "both_strategies": {f["strategy"] for f in fs} == {"snap_to_beat", "beat_only"},
        "three_densities": {f["density"] for f in fs} >= {"low", "medium", "high"},
        **{k: any(f["stats"][k] > 0 for f in snaps) for k in ("snapped", "vad_blocked", "too_far", "low_energy")},
        "non_nearest": any(f["non_nearest"] > 0 for f in fs),
        "min_segment_drop": facts["snap_default_min_segment"]["n_strategy_inside"] < facts["snap_medium"]["n_strategy_inside"],
        "high_adds": facts["snap_high"]["lib_bar_start"] and facts["snap_high"]["n_strategy_inside"] > facts["snap_medium"]["n_strategy_inside"],
        "high_blocks": facts["snap_high"]["stats"]["vad_blocked"] > facts["snap_medium"]["stats"]["vad_blocked"],
        "bo_mdd_verse": any(f["bo_mdd_verse"] for f in fs), "bo_fallback": any(f["bo_fallback"] for f in fs),
        "bo_blocks": any(f["strategy"] == "beat_only" and f["vad_blocked"] > 0 for f in fs),
        "force": any(f["force"] for f in fs), "unprotected": any(f["unprotected"] for f in fs),
        "moved_lib": any(f["moved_lib"] for f in fs), "merge_drops_flag": any(f["merge_drops_flag"] for f in fs),
        "short_lib_survives": any(f["short_lib_survives"] for f in fs),
        "mdd_failed_to_beat_only": any(f["mdd_failed"] and f["strategy"] == "beat_only" for f in fs),
        "unknown_alignment": any(f["configured_alignment"] not in ("snap_to_beat", "beat_only") and f["strategy"] == "snap_to_beat" for f in fs),
        "few_beats": any(f["few_beats"] for f in fs), "stereo": any(f["stereo"] for f in fs),
    }
    print("coverage:", json.dumps(cover, indent=1))
    missing = [k for k, v in cover.items() if not v]
    assert not missing, f"the case set does not cover: {missing}"
    path = HERE / "hybrid_mdd.npz"
    np.savez_compressed(path, versions=json.dumps(MB.VERSIONS), cases=json.dumps(listing), coverage=json.dumps(cover),
                        **{f"min_margin_{k}": v for k, v in mins.items()}, **out)
    print(f"wrote {path.name} ({path.stat().st_size} bytes); min margins: {mins}")


if __name__ == "__main__":
    main()
