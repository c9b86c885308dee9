#!/usr/bin/env python3
"""Generate tests/golden/auto_profile.json by running the reference's own smart-cut layer: `audio_cut.config.auto_profile`
(`resolve_smart_cut_intent`, `derive_alignment_overrides`, `estimate_style`, `build_auto_profile_overrides`),
`audio_cut.config.derive.apply_profile_overrides`, `SeamlessSplitter._apply_smart_cut_runtime` / `_attach_vocal_coverage`
(`src/vocal_smart_splitter/core/seamless_splitter.py:772-893`) and the intent echo of `audio_cut.api.separate_and_segment`.

Runs ONLY where the reference exists; the GPU box never sees it, and no test runs it.  As in make_vpbd_asr_golden.py,
make_beat_golden.py registers the librosa stand-in and the paths.  The splitter's constructor never runs (it reaches for model
downloads): the two methods are called on `object.__new__(SeamlessSplitter)`.

The fixture holds data only: inputs (typed through `profile_cases.encode_value`), seeds, and recorded results, warning categories
and exception classes.  Before anything is written, every style and runtime case must clear each threshold of `estimate_style`
and each tempo anchor by 1e-3, except the comparisons a case lists under `on_threshold`, which must then sit on it exactly.  A case
that misses gets other inputs, never a smaller margin.
"""
from __future__ import annotations

import itertools
import json
import sys
import tempfile
import types
import warnings
import wave
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_beat_golden as MB  # noqa: E402,F401  (registers the librosa stand-in, sets the paths)

from audio_cut_amd import _native  # noqa: E402
from audio_cut_amd.testing import profile_cases as PC  # noqa: E402
from audio_cut.config import auto_profile as ref_ap  # noqa: E402
from audio_cut.config import derive as ref_derive  # noqa: E402
from vocal_smart_splitter.core import seamless_splitter as ref_ss  # noqa: E402
from vocal_smart_splitter.utils import config_manager as ref_cfg  # noqa: E402

MARGIN = 1e-3
THRESHOLDS = {"bpm": (60.0, 88.0, 110.0, 118.0, 122.0, 140.0, 160.0), "energy_cv": (0.25, 0.65),
              "vocal_coverage_ratio": (0.55, 0.68), "global_mdd": (0.45,)}
_ON_NAMES = {"bpm": "bpm", "energy_cv": "cv", "vocal_coverage_ratio": "coverage", "global_mdd": "mdd"}


def _plain(obj):
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


def _recorded(fn):
    """-> {"result" | "error", "warnings"}: what `fn()` returned or the class it raised, and the warning categories in order."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out = {"result": _plain(fn())}
        except Exception as exc:
            out = {"error": type(exc).__name__}
    out["warnings"] = [w.category.__name__ for w in caught]
    return out


def check_margins(features, confidence, on_threshold, label):
    worst = np.inf
    on = set(on_threshold or ())
    for key, marks in THRESHOLDS.items():
        for mark in marks:
            tag = f"{_ON_NAMES[key]}:{mark:g}"
            diff = abs(float(features[key]) - mark)
            if tag in on:
                assert diff == 0.0, (label, tag, features[key])
                on.discard(tag)
                continue
            assert diff >= MARGIN, (label, tag, features[key])
            worst = min(worst, diff)
    assert not on, (label, "unused on_threshold", on)
    assert abs(confidence - 0.6) >= MARGIN
    return float(worst)


# ---- profiles --------------------------------------------------------------------------------------------------------------------
def profiles_block():
    out = {name: _plain(ref_derive.apply_profile_overrides(name)[1]) for name in ("ballad", "pop", "rap", "edm")}
    for name, flat in out.items():
        assert len(flat) == 25, (name, len(flat))
    return {"profiles": out, "default_schema": _plain(ref_derive.build_runtime_override_map(ref_derive.load_default_schema()))}


# ---- intent ----------------------------------------------------------------------------------------------------------------------
def intent_inputs():
    rows = []
    aligns = [None, "lyric", "lyric_lean", "balanced", "beat_lean", "beat", 0.0, 0.3, 0.5, 0.75, 1.0, 1.7, -0.2, "0.4", " Beat "]
    for a in aligns:
        for marked in (False, True):
            sc = {} if a is None else {"alignment": a}
            rows.append((sc, ["smart_cut.alignment"] if marked else []))
    segs = [None, "few", "medium", "many", "4-9", (4, 9), [5.0, 12.0]]
    for s in segs:
        stop = None
        if isinstance(s, str) and s in ref_ap.SEGMENT_DURATION_STOPS:
            stop = list(ref_ap.SEGMENT_DURATION_STOPS[s])
        targets = [None, [5.0, 12.0], [4.0, 10.0]] + ([stop] if stop and stop != [5.0, 12.0] else [])
        for t in targets:
            for marks in ([], ["smart_cut.segments", "smart_cut.target_duration_s"]):
                sc = {}
                if s is not None:
                    sc["segments"] = s
                if t is not None:
                    sc["target_duration_s"] = t
                rows.append((sc, marks))
    for style, a, s, t in itertools.product(("rhythmic", "dense", "natural"), (None, "beat", 0.5), (None, "few"), (None, [4.0, 10.0])):
        sc = {"cut_style": style}
        if a is not None:
            sc["alignment"] = a
        if s is not None:
            sc["segments"] = s
        if t is not None:
            sc["target_duration_s"] = t
        rows.append((sc, []))
        if a == 0.5:
            rows.append((sc, ["smart_cut.alignment"]))
    rows.append(({"segments": "many", "alignment": "beat_lean", "profile": " Rap ", "lyrics": "OFF", "cut_style": "natural",
                  "target_duration_s": [5.0, 12.0]}, []))
    rows.append((dict(ref_cfg.get_config("smart_cut", {})), []))          # the section as the reference's configuration ships it
    for bad in ({"alignment": "loud"}, {"alignment": float("nan")}, {"segments": (9, 4)}, {"segments": (0, 5)}, {"segments": (3, 6, 9)},
                {"segments": "loud"}, {"target_duration_s": (9, 4)}, {"alignment": [0.5]}):
        rows.append((bad, []))
    return rows


def intent_block():
    out = []
    for sc, marks in intent_inputs():
        row = {"smart_cut": PC.encode_value(sc), "explicit_keys": list(marks)}
        rec = _recorded(lambda: ref_ap.resolve_smart_cut_intent(dict(sc), explicit_keys=set(marks)))
        row["intent"] = PC.pack_intent(rec["result"]) if "result" in rec else {"error": rec["error"]}
        row["warnings"] = rec["warnings"]
        apply = _recorded(lambda: ref_ap.should_apply_duration_overrides(dict(sc), explicit_keys=set(marks)))
        row["apply_durations"] = apply.get("result", apply.get("error"))          # True / False, or the exception class
        out.append(row)
    assert any(r["intent"] == {"error": "ValueError"} for r in out)
    assert any("UserWarning" in r["warnings"] for r in out) and any("DeprecationWarning" in r["warnings"] for r in out)
    return out


# ---- alignment -------------------------------------------------------------------------------------------------------------------
CUSTOM_POLES = {"lyric": {"acoustic_pause": 0.5, "beat_affinity": 0.0, "asr_gap": 0.3}, "beat": {"beat_affinity": 0.4, "breath": 0.05}}


def alignment_block():
    out = []
    for name in ("ballad", "pop", "rap", "edm"):
        weights = ref_ap.build_style_weight_overrides(name)
        for a in (0, 0.25, 0.3, 0.4, 0.5, 0.75, 1):
            out.append({"profile": name, "alignment": a, "poles": None,
                        "overrides": PC.pack_alignment(ref_ap.derive_alignment_overrides(a, weights))})
    for a in (0.1, 0.9):
        bare = {k.rsplit(".", 1)[1]: v for k, v in ref_ap.build_style_weight_overrides("pop").items() if "penalty" not in k}
        out.append({"profile": "pop_bare_keys_no_penalties", "alignment": a, "poles": CUSTOM_POLES, "weights": bare,
                    "overrides": PC.pack_alignment(ref_ap.derive_alignment_overrides(a, bare, alignment_poles=CUSTOM_POLES))})
    styles = {f"{name}/{cs}": _plain(ref_ap.build_style_weight_overrides(name, cut_style=cs))
              for name in ("ballad", "pop", "rap", "edm", "polka") for cs in ("natural", "rhythmic", "dense")}
    return {"cases": out, "style_weights": styles}


# ---- style -----------------------------------------------------------------------------------------------------------------------
def style_block():
    out, seen_profiles, seen_anchors, worst = [], set(), set(), np.inf
    for spec in PC.STYLE_CASES:
        est = ref_ap.estimate_style(PC.style_cache(spec))
        worst = min(worst, check_margins(est.features, est.confidence, spec.get("on_threshold"), spec["name"]))
        row = {"name": spec["name"], "estimate": {"profile": est.profile, "confidence": est.confidence, "features": dict(est.features),
                                                  "fallback_reason": est.fallback_reason}}
        for cs in ("natural",):          # the other cut styles change the eight weights only: `alignment.style_weights`
            ov = _plain(ref_ap.build_auto_profile_overrides(est, cut_style=cs))
            ov["meta.auto_profile"] = PC.fold_applied(ov["meta.auto_profile"], applied_keys())
            assert ov["meta.auto_profile"]["applied_overrides"] == PC.APPLIED_MARK
            row[f"overrides_{cs}"] = ov
        out.append(row)
        seen_profiles.add((est.profile, est.fallback_reason))
        seen_anchors.add(tuple(sorted(row["overrides_natural"]["meta.auto_profile"]["anchor_weights"])))
    assert {("ballad", None), ("edm", None), ("rap", None), ("pop", None), ("pop", "low_confidence")} <= seen_profiles, seen_profiles
    assert {("ballad",), ("ballad", "pop"), ("pop", "rap"), ("edm", "rap"), ("edm",), ("pop",)} <= seen_anchors, seen_anchors
    return {"cases": out, "min_margin": worst}


# ---- runtime ---------------------------------------------------------------------------------------------------------------------
def _ref_splitter():
    sp = object.__new__(ref_ss.SeamlessSplitter)
    sp._last_auto_profile_meta = None
    sp._last_intent_meta = None
    return sp


def run_runtime(cache, vocal, dotted, *, marked):
    """The reference's `_apply_smart_cut_runtime` on a fresh configuration holding `dotted`: through `set_runtime_config` (the keys
    count as set by the caller) or written into the tree unmarked, as its API writes its own overrides."""
    ref_cfg.reset_runtime_config()
    if marked:
        ref_cfg.set_runtime_config(dict(dotted))
    else:
        manager = ref_cfg.get_config_manager()
        for key, value in dotted.items():
            manager.set(key, value)
    written = {}
    real = ref_ss.set_runtime_config
    ref_ss.set_runtime_config = lambda ov: (written.update(ov), real(ov))[1]
    sp = _ref_splitter()
    try:
        rec = _recorded(lambda: sp._apply_smart_cut_runtime(cache, vocal_track=vocal))
        if "result" in rec:
            rec = {"meta": PC.fold_applied(rec["result"], applied_keys()), "warnings": rec["warnings"], "intent": _plain(sp._last_intent_meta),
                   "config": {k: _plain(ref_cfg.get_config(k)) for k in sorted(written) if k not in META_KEYS},
                   "meta_in_config": [_plain(ref_cfg.get_config(k)) == want for k, want in
                                      (("meta.auto_profile", rec["result"]), ("meta.intent", _plain(sp._last_intent_meta))) if k in written],
                   "coverage": getattr(cache, "vocal_coverage_ratio", None)}
    finally:
        ref_ss.set_runtime_config = real
        ref_cfg.reset_runtime_config()
    return rec


SAME = "same_as_marked"


def applied_keys():
    """`applied_overrides` of every AutoProfile record: the non-meta keys of a profile map and the eight phrase weights."""
    keys = set(ref_derive.apply_profile_overrides("pop")[1]) | set(ref_ap.build_style_weight_overrides("pop"))
    return sorted(k for k in keys if not k.startswith("meta."))

META_KEYS = ("meta.auto_profile", "meta.intent")      # what `get_config` returns for them is the two records: compared, not stored twice


def _both(row, marked, unmarked):
    """The two runs of a case; of the unmarked one what differs (`profile_cases.delta`)."""
    row.update({"marked": marked, "unmarked": SAME if unmarked == marked else PC.delta(marked, unmarked)})
    return row


def runtime_block():
    ns = types.SimpleNamespace
    unit = {}
    # the cases of the reference's tests/unit/test_seamless_splitter_auto_profile.py and test_seamless_splitter_intent_runtime.py
    rap = lambda **kw: ns(bpm_features=ns(main_bpm=142.0), global_mdd=0.58, rms_series=np.asarray([0.40, 0.52, 0.47], dtype=np.float32), **kw)
    pop = lambda: ns(bpm_features=ns(main_bpm=108.0), global_mdd=0.38, rms_series=np.asarray([0.2, 0.42, 0.31], dtype=np.float32),
                     vocal_coverage_ratio=0.56, beat_times=np.asarray([0.0, 0.5, 1.0], dtype=np.float32))
    table = {
        "auto_rhythmic_target": (lambda: rap(vocal_coverage_ratio=0.82), None,
                                 {"smart_cut.profile": "auto", "smart_cut.cut_style": "rhythmic", "smart_cut.target_duration_s": [4.0, 10.0]}),
        "manual_ballad": (lambda: rap(vocal_coverage_ratio=0.82), None, {"smart_cut.profile": "ballad", "smart_cut.target_duration_s": [5.0, 12.0]}),
        "coverage_from_ones": (lambda: rap(), "ones", {"smart_cut.profile": "auto"}),
        "beat_many": (pop, "zeros", {"smart_cut.alignment": "beat", "smart_cut.segments": "many"}),
        "balanced": (pop, "zeros", {"smart_cut.alignment": "balanced"}),
    }
    for name, (make, vocal_kind, dotted) in table.items():
        vocal = None if vocal_kind is None else (np.ones if vocal_kind == "ones" else np.zeros)(44100, dtype=np.float32)
        unit[name] = _both({"vocal": vocal_kind, "smart_cut": PC.encode_value(dotted)},
                           run_runtime(make(), vocal, dotted, marked=True), run_runtime(make(), vocal, dotted, marked=False))
    seeded, worst = [], np.inf
    for spec in PC.SMART_CUT_CASES:
        recs = []
        for marked in (True, False):
            cache, _, vocal, _ = PC.smart_cut_case(spec)
            rec = run_runtime(cache, vocal, spec["smart_cut"], marked=marked)
            assert "error" not in rec, (spec, rec)
            recs.append(rec)
            if rec["meta"] is not None:
                worst = min(worst, check_margins(rec["meta"]["features"], rec["meta"]["confidence"], None, spec["seed"]))
        seeded.append(_both({"seed": spec["seed"]}, *recs))
    assert sum(r["marked"]["meta"] is not None for r in seeded) >= 4 and any(r["marked"]["meta"] is None for r in seeded)
    assert any(r["unmarked"] != SAME for r in seeded) or any(u["unmarked"] != SAME for u in unit.values())
    return {"auto_applied_overrides": applied_keys(), "unit": unit, "seeded": seeded, "min_margin": worst}


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def coverage_block():
    sp, out = _ref_splitter(), []
    for recipe, n, seed in PC.coverage_cases(_native.PROFILE_GRID_SAMPLES):
        x = PC.coverage_signal(recipe, n, seed)
        cache = types.SimpleNamespace()
        sp._attach_vocal_coverage(cache, x)
        coverage = cache.vocal_coverage_ratio
        # the intermediate values of the same lines of the reference (`:884-889`), recorded beside its result
        peak = float(np.max(np.abs(x)))
        thr = np.float32(max(peak * 0.03, 1e-5))
        count = int(np.count_nonzero(np.abs(x) >= max(peak * 0.03, 1e-5)))
        assert coverage == (0.0 if peak <= 1e-9 else count / n), (recipe, n)
        out.append({"recipe": recipe, "n": n, "seed": seed, "peak": peak, "peak_bits": int(np.float32(peak).view(np.uint32)),
                    "thr_bits": int(thr.view(np.uint32)), "count": count, "coverage": coverage})
    by = {(r["recipe"], r["n"]): r for r in out}
    assert by[("peak_5e-10", 4097)]["coverage"] == 0.0 and by[("peak_5e-10", 4097)]["count"] == 0
    assert by[("peak_2e-9", 4097)]["count"] == 0 and by[("peak_2e-9", 4097)]["peak"] > 1e-9
    assert 0.3 < by[("noise_half", 4097)]["coverage"] < 0.7
    r = by[("thr_rounds_down", 4097)]
    assert float(np.uint32(r["thr_bits"]).view(np.float32)) < r["peak"] * 0.03      # the rounded threshold is the smaller one
    return out


# ---- api -------------------------------------------------------------------------------------------------------------------------
def api_block():
    from audio_cut import api as ref_api
    calls = []

    class FakeSplitter:
        def __init__(self, sample_rate):
            self.sample_rate = sample_rate

        def split_audio_seamlessly(self, input_file, output_dir, *, mode, export_plan=None):
            calls.append(mode)
            return {"success": True, "method": f"pure_vocal_split_{mode}", "export_plan": [], "cut_points_sec": [0.0, 2.0],
                    "cut_points_samples": [0, 88200], "segment_labels": ["human"], "segment_durations": [2.0], "segment_vocal_flags": [True]}

    real, ref_api.SeamlessSplitter = ref_api.SeamlessSplitter, FakeSplitter
    out = []
    pairs = [("medium", 0.75, None), ("many", "beat", None), (None, None, None), ("few", None, None), (None, "lyric_lean", None),
             ((4, 9), 0.3, None), ("many", "beat_lean", None), ("few", "beat", "hybrid_mdd"), (None, 0.5, None), ("medium", None, "vpbd_acoustic")]
    try:
        with tempfile.TemporaryDirectory() as tmp:
            src = Path(tmp) / "song.wav"
            with wave.open(str(src), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(44100); w.writeframes(bytes(2 * 44100 * 2))
            for segments, alignment, mode in pairs:
                ref_cfg.reset_runtime_config()
                man = ref_api.separate_and_segment(input_uri=str(src), export_dir=str(Path(tmp) / "out"), segments=segments,
                                                   alignment=alignment, mode=mode)
                out.append({"segments": PC.encode_value(segments), "alignment": alignment, "mode": mode, "called_mode": calls[-1],
                            "version": man["version"], "intent": _plain(man.get("intent"))})
    finally:
        ref_api.SeamlessSplitter = real
        ref_cfg.reset_runtime_config()
    assert [r["called_mode"] for r in out[:3]] == ["vpbd_asr", "vpbd_asr", "v2.2_mdd"] and out[2]["intent"] is None
    return out


def main() -> None:
    blocks = {"versions": {"numpy": np.__version__}, **profiles_block(), "intent": intent_block(), "alignment": alignment_block(),
              "style": style_block(), "runtime": runtime_block(), "coverage": coverage_block(), "api": api_block()}
    path = HERE / "auto_profile.json"
    rows = [f"{json.dumps(k)}: {json.dumps(v, ensure_ascii=False)}" for k, v in blocks.items()]         # one block per line
    path.write_text("{\n" + ",\n".join(rows) + "\n}\n", encoding="utf-8")
    print("wrote", path.name, path.stat().st_size, "bytes;", len(blocks["intent"]), "intent rows,", len(blocks["coverage"]),
          "coverage cases; min margins", blocks["style"]["min_margin"], blocks["runtime"]["min_margin"])


if __name__ == "__main__":
    main()
