#!/usr/bin/env python3
"""Generate tests/golden/vpbd_asr.json by running the reference's own lyrics path: `VocalPhraseBoundaryDetector.detect` with the
`fake` provider (`src/vocal_smart_splitter/core/vocal_phrase_boundary_detector.py:49-183`), `LyricsTimeline.from_dict`, the four
`vpbd_asr` hooks of `_process_pure_vocal_split` (`seamless_splitter.py:484-493,547-551,575-584,624-628`),
`attach_lyrics_to_segments` / `_build_manifest`, and the two scenarios of its integration test
(`tests/integration/test_pipeline_vpbd_asr_fake_provider.py`) - over the oracle's librosa restatement.

Runs ONLY where the reference exists (/root/reference); the GPU box never sees it.  As in make_hybrid_golden.py,
`oracle.librosa_ops` is registered under the name `librosa` (through make_beat_golden.py) and `soundfile` is an empty stand-in:
the reference module's `_write_asr_vocal_copy` is replaced by a recorder, so no WAV is written here (libsoxr and libsndfile are
absent; the WAV's bytes are pinned by the GPU tests against the oracle's resampler and `pcm_bytes_host`).

The fixture holds data only: seeds, configuration overrides, timelines and recorded results.  Before anything is written
  * every candidate source appears among the selected candidates of some case, as the winner or merged into a selected cluster;
  * at least one cluster merges a lyrics and an acoustic candidate;
  * at least one restore happens in the guard-restore cases;
  * no decision of the lyrics features sits on a knife edge: every comparison of a candidate time with a word edge, a word-edge
    tolerance or a sentence tolerance, every word gap against 0.35 s / 1.5 s and every confidence against 0.85 either compares a
    value with a copy of itself (difference exactly 0: a sentence-end candidate against that sentence's end) or clears its
    threshold by 1e-6.  A case that misses gets another seed, never a smaller margin.
"""
from __future__ import annotations

import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_beat_golden as MB  # noqa: E402,F401  (registers the librosa stand-in, sets the paths)

from audio_cut_amd.testing.lyrics_cases import CASE_SECONDS, asr_case  # noqa: E402
from audio_cut_amd.testing.vpbd_inputs import FixedPauses  # noqa: E402
from audio_cut.lyrics.models import LyricsTimeline as RefTimeline  # noqa: E402
from audio_cut.lyrics.segment_attach import attach_lyrics_to_segments as ref_attach  # noqa: E402
from audio_cut.cutting.refine import CutAdjustment as RefAdjustment  # noqa: E402
from vocal_smart_splitter.core import seamless_splitter as ref_ss  # noqa: E402
from vocal_smart_splitter.core import vocal_phrase_boundary_detector as ref_vpbd  # noqa: E402
from vocal_smart_splitter.utils import config_manager as ref_cfg  # noqa: E402

SR = 44100
MARGIN = 1e-6
FIXTURE_KEY = "lyrics_alignment.fixture_path"
NO_DEBUG = "vpbd.candidate_debug_json"
REF_SIMPLE = MB.REF / "tests" / "fixtures" / "lyrics" / "simple_song_timeline.json"
LYRICS_SOURCES = ("lyrics_gap", "sentence_end", "mvad_boundary")
ACOUSTIC_SOURCES = ("acoustic_pause", "breath", "mdd_valley")

_asr_calls = []


def _record_asr_copy(*, vocal_track, output_dir, input_path, source_sample_rate):
    _asr_calls.append((len(vocal_track), str(output_dir), str(input_path), int(source_sample_rate)))
    return Path(output_dir) / f"{Path(input_path).stem}_vocal_for_asr.wav"


ref_vpbd._write_asr_vocal_copy = _record_asr_copy


def _plain(obj):
    """JSON round trip: what the test will compare with (float keys become strings, tuples lists)."""
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


def run_detect(overrides, timeline_payload, *, cache, pauses, vocal, sr=SR, input_path="track.wav", mode="vpbd_asr"):
    """-> {"boundary_detection", "lyrics_alignment"} or {"error", "message"}.  `timeline_payload` None: the fixture path of the
    overrides is used as it stands (a missing file)."""
    with tempfile.TemporaryDirectory() as tmp:
        ov = dict(overrides)
        if timeline_payload is not None:
            path = Path(tmp) / "timeline.json"
            path.write_text(json.dumps(timeline_payload, ensure_ascii=False), encoding="utf-8")
            ov[FIXTURE_KEY] = str(path)
        ref_cfg.reset_runtime_config()
        ref_cfg.set_runtime_config(ov)
        try:
            res = ref_vpbd.VocalPhraseBoundaryDetector(sr).detect(
                mode=mode, vocal_track=vocal, original_audio=vocal, pure_vocal_detector=FixedPauses(pauses), feature_cache=cache,
                vad_segments=None, input_path=input_path, output_dir=str(Path(tmp) / "out"))
        except Exception as exc:
            return {"error": type(exc).__name__, "message": str(exc).replace(tmp, "<tmp>")}, None
        finally:
            ref_cfg.reset_runtime_config()
    return _plain({"boundary_detection": res.boundary_detection, "lyrics_alignment": res.lyrics_alignment}), res


def knife_edges(payload, candidate_times, *, tol_ms=60.0):
    """Smallest margin over every comparison the lyrics features and the candidate generator take (0-differences of copies excluded)."""
    worst = np.inf

    def clear(diff):
        nonlocal worst
        if diff != 0.0:
            worst = min(worst, abs(diff))
    tl = RefTimeline.from_dict(payload, strict=True)
    for a, b in zip(tl.words, tl.words[1:]):
        gap = b.start_s - a.end_s
        clear(gap - 0.35); clear(gap - 1.5)
    for item in list(tl.words) + list(tl.vad_regions) + list(tl.sentences):
        if item.confidence is not None:
            clear(item.confidence - 0.85)
    tol = tol_ms / 1000.0
    for t in candidate_times:
        for w in tl.words:
            clear(t - w.start_s); clear(t - w.end_s)
            if w.start_s < t < w.end_s:
                clear(min(t - w.start_s, w.end_s - t) - tol)
        for r in tl.vad_regions:
            clear(t - r.start_s); clear(t - r.end_s)
        for s in tl.sentences:
            clear(abs(t - s.end_s) - 0.25)
    return float(worst)


def detect_cases():
    plans = [("unified", False), ("unified", True), ("legacy", False), ("unified", True), ("legacy", True), ("unified", False)]
    out, seed = [], 41
    for pool, beats in plans:
        while True:
            cache, pauses, vocal, payload = asr_case(seed, breaths=beats)        # the cases with beat candidates also carry breaths
            overrides = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", "lyrics_alignment.strict": False,
                         NO_DEBUG: False, "vpbd.candidate_pool": pool, "vpbd.beat_candidates.enable": beats}
            if beats:                 # a denser plan, so that weak sources (beats, breaths) get selected somewhere
                overrides.update({"global_planner.hard_min_s": 1.0, "global_planner.target_min_s": 2.0, "global_planner.target_max_s": 4.0,
                                  "global_planner.hard_max_s": 6.0})
            n_calls = len(_asr_calls)
            rec, res = run_detect(overrides, payload, cache=cache, pauses=pauses, vocal=vocal)
            assert res is not None, rec
            assert len(_asr_calls) == n_calls + 1 and _asr_calls[-1][0] == len(vocal) and _asr_calls[-1][3] == SR
            bd = rec["boundary_detection"]
            times = [c["t"] for c in bd["selected"] + bd["suppressed"]]
            margin = knife_edges(payload, times)
            seed += 1
            if margin >= MARGIN:
                break
            print(f"  seed {seed - 1}: margin {margin:.2e} < {MARGIN:g}, next seed")
        assert bd["actual_mode"] == "vpbd_asr" and rec["lyrics_alignment"]["fallback_reason"] is None
        print(f"  detect seed {seed - 1} pool={pool} beats={beats}: counts {bd['candidate_counts']} margin {margin:.2e}")
        out.append({"seed": seed - 1, "breaths": bool(beats), "overrides": overrides, "margin": margin, "result": rec})     # inputs: lyrics_cases.asr_case(seed, breaths)
    return out


def fallback_cases():
    seed = 31
    cache, pauses, vocal, good = asr_case(seed)
    beyond = json.loads(json.dumps(good))
    beyond["words"].append({"text": "late", "start_s": CASE_SECONDS - 0.5, "end_s": CASE_SECONDS + 1.25, "confidence": 0.9})
    beyond["sentences"].append({"text": "late", "start_s": CASE_SECONDS - 0.5, "end_s": CASE_SECONDS + 1.25, "confidence": 0.9})
    base = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", NO_DEBUG: False}
    missing = {FIXTURE_KEY: "no_such_dir/missing_timeline.json"}
    specs = [("missing_fixture", dict(base, **missing, **{"lyrics_alignment.strict": False}), None),
             ("missing_fixture_strict", dict(base, **missing, **{"lyrics_alignment.strict": True}), None),
             ("beyond_duration", dict(base, **{"lyrics_alignment.strict": False}), beyond),
             ("beyond_duration_strict", dict(base, **{"lyrics_alignment.strict": True}), beyond),
             ("cli_unconfigured", {NO_DEBUG: False, "lyrics_alignment.enabled": True, "lyrics_alignment.provider": "cli", "lyrics_alignment.strict": False}, None)]
    # The candidates of a fallback are not recorded a second time: the reference itself gives those of the run it falls back to -
    # the acoustic pool (`vpbd_acoustic` on the same inputs), or for the over-long interval the run on the timeline without it.
    kw = dict(cache=cache, pauses=pauses, vocal=vocal)
    same_as = {"acoustic": run_detect({NO_DEBUG: False}, None, mode="vpbd_acoustic", **kw)[0],
               "good_timeline": run_detect(dict(base, **{"lyrics_alignment.strict": False}), good, **kw)[0]}
    twin = {"missing_fixture": "acoustic", "beyond_duration": "good_timeline", "cli_unconfigured": "acoustic"}
    out = []
    for name, overrides, payload in specs:
        rec, _ = run_detect(overrides, payload, **kw)
        if "error" not in rec:
            for key in ("selected", "suppressed"):
                assert rec["boundary_detection"].pop(key) == same_as[twin[name]]["boundary_detection"][key], (name, key)
            rec["candidates_as"] = twin[name]
        print(f"  fallback {name}: " + (f"{rec['error']}: {rec['message']}" if "error" in rec else
                                        f"{rec['boundary_detection']['actual_mode']} / {rec['lyrics_alignment']['fallback_reason']} / "
                                        f"{rec['lyrics_alignment']['warnings']}"))
        out.append({"name": name, "seed": seed, "overrides": overrides, "timeline": payload, "result": rec})
    assert "error" in out[1]["result"] and "error" in out[3]["result"] and out[4]["result"]["lyrics_alignment"]["fallback_reason"] == "lyrics_alignment_unavailable"
    return out


def from_dict_cases():
    w = lambda **k: dict({"text": "a", "start_s": 1.0, "end_s": 1.5, "confidence": 0.9}, **k)
    payloads = [
        ("valid", {"duration_s": 10.0, "source": "x", "words": [w(), w(text="b", start_s=0.2, end_s=0.6, confidence=None)],
                   "sentences": [{"text": "b a.", "start_s": 0.2, "end_s": 1.5}], "vad_regions": [{"start_s": 0.1, "end_s": 1.6, "kind": ""}],
                   "meta": {"engine": "test"}, "warnings": ["w0"]}),
        ("no_duration", {"words": [w(end_s=1e6)]}),
        ("overshoot_clamped", {"duration_s": 10.0, "words": [w(start_s=9.5, end_s=10.0009)], "sentences": [{"text": "s", "start_s": 9.0, "end_s": 10.0004}]}),
        ("overshoot_too_far", {"duration_s": 10.0, "words": [w(start_s=9.5, end_s=10.002)]}),
        ("overshoot_start_past_end", {"duration_s": 10.0, "vad_regions": [{"start_s": 10.0, "end_s": 10.0005}]}),
        ("negative_start", {"duration_s": 10.0, "words": [w(start_s=-0.1)]}),
        ("end_before_start", {"duration_s": 10.0, "words": [w(), w(start_s=2.0, end_s=2.0)]}),
        ("confidence_range", {"duration_s": 10.0, "words": [w(confidence=1.2)], "vad_regions": [{"start_s": 0.0, "end_s": 1.0, "confidence": -0.1}]}),
        ("confidence_text", {"duration_s": 10.0, "words": [w(confidence="high")]}),
        ("start_missing", {"duration_s": 10.0, "sentences": [{"text": "s", "end_s": 1.0}]}),
        ("empty_text", {"duration_s": 10.0, "words": [w(text="")], "sentences": [{"text": "", "start_s": 0.0, "end_s": 1.0}]}),
        ("zero_duration", {"duration_s": 0.0}),
        ("duration_text", {"duration_s": "long"}),
        ("empty", {}),
    ]
    out = []
    for name, payload in payloads:
        for strict in (False, True):
            try:
                rec = {"timeline": RefTimeline.from_dict(json.loads(json.dumps(payload)), strict=strict).to_dict()}
            except Exception as exc:
                rec = {"error": type(exc).__name__, "message": str(exc)}
            out.append({"name": name, "strict": strict, "payload": payload, "result": _plain(rec)})
    assert any("error" in c["result"] for c in out) and any("clamped" in " ".join(c["result"].get("timeline", {}).get("warnings", [])) for c in out)
    return out


def _ref_splitter(sr=SR):
    fake = object.__new__(ref_ss.SeamlessSplitter)
    fake.sample_rate = sr
    return fake


def restore_cases():
    words = [(1.0, 1.5), (1.6, 2.4), (5.0, 5.6), (9.0, 9.7), (12.0, 12.6)]
    n = 15 * SR
    adj = lambda raw, final, score=0.8: [raw, final, final, score, (final - raw) * 1000.0, (final - raw) * 1000.0]
    sm = lambda t: int(round(t * SR))
    specs = [
        ("restore", [0, sm(5.2), sm(10.0), n], [adj(4.8, 5.2), adj(10.0, 10.0)], 1.0),
        ("restore_two", [0, sm(2.0), sm(5.2), sm(9.3), n], [adj(2.5, 2.0), adj(4.8, 5.2), adj(8.8, 9.3)], 1.0),
        ("min_gap_refuses", [0, sm(4.2), sm(5.2), n], [adj(4.8, 5.2)], 1.0),
        ("min_gap_zero_allows", [0, sm(4.2), sm(5.2), n], [adj(4.8, 5.2)], 0.0),
        ("raw_at_zero", [0, sm(1.2), n], [adj(0.0, 1.2)], 1.0),
        ("raw_at_end", [0, sm(12.3), n], [adj(15.0, 12.3)], 1.0),
        ("raw_inside_word", [0, sm(5.2), n], [adj(5.5, 5.2)], 1.0),
        ("final_outside_word", [0, sm(4.0), n], [adj(5.2, 4.0)], 1.0),
        ("final_not_a_boundary", [0, sm(7.0), n], [adj(4.8, 5.2)], 1.0),
        ("no_words", [0, sm(5.2), n], [adj(4.8, 5.2)], 1.0),
        ("no_adjustments", [0, sm(5.2), n], [], 1.0),
    ]
    out, fake = [], _ref_splitter()
    for name, points, adjs, min_gap in specs:
        iv = [] if name == "no_words" else words
        got_points, got_adj = fake._restore_guard_points_outside_lyrics_words(
            list(points), [RefAdjustment(*a) for a in adjs], list(iv), sample_count=n, min_gap_s=min_gap)
        rec = {"points": [int(p) for p in got_points],
               "adjustments": None if got_adj is None else [[a.raw_time, a.guard_time, a.final_time, a.score, a.guard_shift_ms, a.final_shift_ms] for a in got_adj]}
        out.append({"name": name, "points": points, "adjustments": adjs, "word_intervals": [list(x) for x in iv], "sample_count": n,
                    "min_gap_s": min_gap, "result": _plain(rec)})
    by = {c["name"]: c["result"] for c in out}
    assert by["restore"]["adjustments"] is not None and sm(4.8) in by["restore"]["points"]
    assert by["min_gap_refuses"]["adjustments"] is None and by["raw_at_zero"]["adjustments"] is None and by["raw_inside_word"]["adjustments"] is None
    return out


def collect_cases():
    inputs = [
        None, {}, {"timeline": None}, {"timeline": []}, "text",
        {"timeline": {"words": None, "sentences": None, "vad_regions": None}},
        {"timeline": {"words": [{"start_s": 1.0, "end_s": 1.4}, {"start_s": 1.0, "end_s": 1.4}, {"start_s": "2", "end_s": "2.5"}, "junk",
                                {"start_s": 3.0, "end_s": 3.0}, {"start_s": 5.0, "end_s": 4.0}, {"start_s": None, "end_s": 1.0}, {"end_s": 2.0},
                                {"start_s": "x", "end_s": 1.0}, {"start_s": 0.2, "end_s": 0.4}],
                      "sentences": [{"end_s": 2.4}, {"end_s": 2.4}, {"end_s": 0.0}, {"end_s": -1.0}, {"end_s": "7.5"}, {"end_s": None}, 17, {"start_s": 1.0}],
                      "vad_regions": [{"start_s": 0.9, "end_s": 2.5, "kind": "singing"}, {"start_s": 0.0, "end_s": 0.9}, {"start_s": "bad", "end_s": 6.0},
                                      None, {"end_s": 2.4}]}},
        {"timeline": asr_case(41)[3]},
    ]
    out = []
    for item in inputs:
        out.append({"input": item,
                    "word_intervals": _plain(ref_ss.SeamlessSplitter._collect_lyrics_word_intervals(item)),
                    "boundary_times": _plain(ref_ss.SeamlessSplitter._collect_lyrics_boundary_times(item))})
    return out


def attach_cases():
    from audio_cut import api as ref_api
    payload = asr_case(41)[3]
    tl = RefTimeline.from_dict(payload, strict=True)
    cjk = [s for s in tl.sentences if s.text.endswith("。")][0]
    edges = sorted({0.0, CASE_SECONDS, cjk.start_s - 0.2, cjk.end_s + 0.2, tl.words[4].start_s + 0.5 * (tl.words[4].end_s - tl.words[4].start_s) + 0.013,
                    tl.words[9].start_s + 0.1, 12.0})
    segments = [{"id": f"{i + 1:04d}", "start": a, "end": b, "label": "human"} for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    segments += [{"id": "bad1", "start": None, "end": 3.0}, {"id": "bad2", "start": 5.0, "end": 5.0}, {"id": "bad3", "start": "x", "end": 9.0},
                 {"id": "text", "start": "1.0", "end": "4.0"}]
    out = {"timeline": payload, "segments": segments, "attached": _plain(ref_attach(segments, tl))}
    result = {"success": True, "cut_points_sec": edges, "segment_labels": ["human" if i % 2 == 0 else "music" for i in range(len(edges) - 1)],
              "segment_durations": [b - a for a, b in zip(edges[:-1], edges[1:])], "cut_points_samples": [int(round(e * SR)) for e in edges],
              "lyrics_alignment": {"enabled": True, "provider": "fake", "strict": False, "fallback_reason": None, "timeline": tl.to_dict()}}
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "song.wav"
        src.write_bytes(b"RIFF")
        man = ref_api._build_manifest(result=result, input_path=src, export_dir=Path(tmp) / "out", mode="vpbd_asr", sample_rate=SR, channels=1,
                                      layout_cfg={})
    result["lyrics_alignment"]["timeline"] = None             # the test puts `timeline` back: not recorded twice
    out["manifest_result"] = _plain(result)
    out["manifest_segments"] = _plain(man["segments"])
    assert any(s.get("lyrics") for s in out["manifest_segments"]) and any(s.get("lyrics") is None for s in out["manifest_segments"])
    joined = [s["lyrics"]["text"] for s in out["attached"] if s["lyrics"]]
    assert any(" " not in t and len(t) > 1 for t in joined) and any(" " in t for t in joined)       # the CJK joiner and the space joiner
    return out


PRIORITY_TIMELINE = {
    "duration_s": 8.0, "source": "fake",
    "words": [{"text": "lead", "start_s": 0.50, "end_s": 0.90, "confidence": 0.95}, {"text": "hold", "start_s": 1.00, "end_s": 2.30, "confidence": 0.93},
              {"text": "line", "start_s": 3.80, "end_s": 4.40, "confidence": 0.91}],
    "sentences": [{"text": "lead hold", "start_s": 0.50, "end_s": 2.30, "confidence": 0.94}, {"text": "line", "start_s": 3.80, "end_s": 4.40, "confidence": 0.91}],
    "vad_regions": [{"start_s": 0.45, "end_s": 2.35, "confidence": 0.90, "kind": "singing"}, {"start_s": 3.75, "end_s": 4.40, "confidence": 0.87, "kind": "singing"}]}
INTEGRATION_CONFIG = {       # the reference test's own, plus the switch that keeps the candidate debug file (a path) out of the results
    NO_DEBUG: False,
    "gpu_pipeline.enable": False, "segment_layout.enable": False, "quality_control.enforce_quiet_cut.enable": False,
    "quality_control.local_boundary_refine.enable": False, "quality_control.pure_music_min_duration": 0.0, "quality_control.min_split_gap": 1.0,
    "global_planner.hard_min_s": 1.0, "global_planner.hard_max_s": 6.0, "global_planner.target_min_s": 2.0, "global_planner.target_max_s": 5.0,
    "lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", "lyrics_alignment.strict": True}
PRIORITY_CONFIG = dict(INTEGRATION_CONFIG, **{
    "vpbd.candidate_pool": "unified", "vpbd.breath_score_scale": 0.6, "vpbd.beat_candidates.enable": True, "vpbd.beat_candidates.bars_per_cut": 1,
    "vpbd.beat_candidates.base_score": 0.3, "global_planner.vocal_risk_weight": 0.0, "global_planner.beat_conflict_weight": 0.0})
SIMPLE_PAUSES = [dict(start_time=5.3, end_time=5.7, cut_point=5.5, confidence=0.6, duration=0.4)]
PRIORITY_PAUSES = [dict(start_time=4.34, end_time=4.46, cut_point=4.4, confidence=1.0, duration=0.12, pause_type="breath"),
                   dict(start_time=5.3, end_time=5.7, cut_point=5.5, confidence=1.0, duration=0.4, pause_type="true_pause")]


def integration_cases():
    """The reference's integration test, scenario for scenario: (1) the whole `_process_pure_vocal_split` on 8 s of silence with its
    fake separator and one pause, (2) `detect` at 16 kHz with a breath, a long pause and beat candidates."""
    simple = json.loads(REF_SIMPLE.read_text(encoding="utf-8"))
    (HERE / "simple_song_timeline.json").write_text(REF_SIMPLE.read_text(encoding="utf-8"), encoding="utf-8")
    out = {}
    # scenario 1
    from vocal_smart_splitter.core.enhanced_vocal_separator import SeparationResult
    from vocal_smart_splitter.core.utils.result_builder import ResultBuilder
    audio = np.zeros(SR * 8, dtype=np.float32)
    fake = _ref_splitter()
    fake._export_format, fake._export_options, fake._precision_guard_ok = "wav", {}, True
    fake._last_segment_classification_debug = []
    fake._last_guard_shift_stats = fake._blank_guard_stats()
    fake._last_guard_adjustments, fake._last_guard_adjustments_raw, fake._last_suppressed_cut_points = [], [], []
    fake._last_auto_profile_meta = fake._last_intent_meta = None
    fake._load_and_resample_if_needed = lambda path: audio
    fake._apply_smart_cut_runtime = lambda *a, **k: None        # AutoProfile / intent overrides are product policy: the base configuration runs
    fake.separator = types.SimpleNamespace(separate_for_detection=lambda a, gpu_context=None: SeparationResult(
        vocal_track=np.asarray(a, dtype=np.float32), instrumental_track=np.zeros_like(a, dtype=np.float32), separation_confidence=1.0,
        backend_used="fake", processing_time=0.0, quality_metrics={}, feature_cache=None, vad_segments=[], gpu_meta={"gpu_pipeline_used": False}))
    fake.pure_vocal_detector = FixedPauses([types.SimpleNamespace(**p) for p in SIMPLE_PAUSES])
    fake.vpbd_detector = ref_vpbd.VocalPhraseBoundaryDetector(SR)
    fake.segment_exporter = types.SimpleNamespace(export_segments=lambda *a, **k: [], export_full_track=lambda *a, **k: "")
    fake.result_builder = ResultBuilder(precision_guard_avg_ms=ref_ss.PRECISION_GUARD_AVG_MS, precision_guard_p95_ms=ref_ss.PRECISION_GUARD_P95_MS)
    with tempfile.TemporaryDirectory() as tmp:
        ref_cfg.reset_runtime_config()
        ref_cfg.set_runtime_config(dict(INTEGRATION_CONFIG, **{FIXTURE_KEY: str(REF_SIMPLE)}))
        try:
            res = fake._process_pure_vocal_split(str(Path(tmp) / "song.wav"), str(Path(tmp) / "out"), "vpbd_asr", export_plan=("none",))
        finally:
            ref_cfg.reset_runtime_config()
    assert res["success"] is True and res["boundary_detection"]["actual_mode"] == "vpbd_asr" and res["lyrics_alignment"]["word_count"] == 3
    assert res["lyrics_cut_protection_applied"] is False
    assert {c["source"] for c in res["boundary_detection"]["selected"]} & set(LYRICS_SOURCES)
    out["simple"] = {"config": INTEGRATION_CONFIG, "timeline": simple, "pauses": SIMPLE_PAUSES, "seconds": 8.0, "sample_rate": SR,
                     "result": _plain({k: res[k] for k in ("boundary_detection", "lyrics_alignment", "lyrics_cut_protection_applied",
                                                           "cut_points_samples", "segment_vocal_flags", "segment_layout_applied")})}
    print(f"  integration simple: cuts {res['cut_points_samples']} counts {res['boundary_detection']['candidate_counts']}")
    # scenario 2
    cache = types.SimpleNamespace(beat_times=np.arange(0.0, 8.001, 0.5, dtype=np.float32), rms_series=np.full(160, 0.8, dtype=np.float32),
                                  hop_s=0.05, duration_s=8.0, mdd_series=np.full(160, 0.5, dtype=np.float32))
    rec, res2 = run_detect(PRIORITY_CONFIG, PRIORITY_TIMELINE, cache=cache, pauses=[types.SimpleNamespace(**p) for p in PRIORITY_PAUSES],
                           vocal=np.zeros(16000 * 8, dtype=np.float32), sr=16000, input_path="sample.wav")
    assert res2 is not None, rec
    assert rec["boundary_detection"]["candidate_counts"]["beat"] > 0
    out["priority"] = {"config": PRIORITY_CONFIG, "timeline": PRIORITY_TIMELINE, "pauses": PRIORITY_PAUSES, "seconds": 8.0, "sample_rate": 16000,
                       "result": rec}
    print(f"  integration priority: counts {rec['boundary_detection']['candidate_counts']}")
    return out


def main() -> None:
    print("vpbd_asr golden")
    detect = detect_cases()
    fixture = {"detect": detect, "fallbacks": fallback_cases(), "from_dict": from_dict_cases(), "restore": restore_cases(),
               "collect": collect_cases(), "attach": attach_cases(), "integration": integration_cases()}
    # coverage
    selected_sources, merged_mixed = set(), 0
    for case in detect + [fixture["integration"]["priority"], fixture["integration"]["simple"]]:
        bd = case["result"]["boundary_detection"]
        for c in bd["selected"]:          # a selected cluster carries every source that merged into it
            selected_sources.update([c["source"]] + list(c.get("meta", {}).get("sources", [])))
        for c in bd["selected"] + bd["suppressed"]:
            srcs = set(c.get("meta", {}).get("sources", []))
            merged_mixed += bool(srcs & set(LYRICS_SOURCES)) and bool(srcs & set(ACOUSTIC_SOURCES))
    wanted = {"acoustic_pause", "breath", "beat", "lyrics_gap", "sentence_end", "mvad_boundary"}
    assert wanted <= selected_sources, (wanted - selected_sources)
    assert merged_mixed >= 1
    pools = [c["overrides"]["vpbd.candidate_pool"] for c in detect]
    assert len(detect) == 6 and "legacy" in pools and "unified" in pools and sum(bool(c["overrides"]["vpbd.beat_candidates.enable"]) for c in detect) >= 2
    assert all(c["result"]["boundary_detection"]["candidate_counts"]["lyrics_pooled"] == 0 for c in detect if c["overrides"]["vpbd.candidate_pool"] == "legacy")
    path = HERE / "vpbd_asr.json"             # one section per line: a later change shows which section moved
    rows = [f"{json.dumps(k)}:{json.dumps(v, ensure_ascii=False, separators=(',', ':'))}" for k, v in fixture.items()]
    path.write_text("{\n" + ",\n".join(rows) + "\n}\n", encoding="utf-8")
    print(f"wrote {path} ({path.stat().st_size / 1024:.0f} KiB): sources {sorted(selected_sources)}, {merged_mixed} lyrics+acoustic clusters")


if __name__ == "__main__":
    main()
