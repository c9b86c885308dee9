"""Seeded inputs for the smart-cut intent / AutoProfile layer (tests + golden generation, tests/golden/auto_profile.json):
signals for the vocal-coverage kernel (`ac_abs_peak_coverage`), feature caches that land in every branch of `estimate_style`, and
runtime cases built on `lyrics_cases.asr_case`.  Data and generators only; the expected values are recorded from the reference."""
from __future__ import annotations

import math
import types
from typing import Any, Dict, List, Tuple

import numpy as np

from .lyrics_cases import asr_case

F32 = np.float32


# ---- JSON carriage of inputs whose Python type matters (a tuple is hashable, a list is not; nan is no JSON) -------------------------
def encode_value(v: Any) -> Any:
    if isinstance(v, tuple):
        return {"__tuple__": [encode_value(x) for x in v]}
    if isinstance(v, list):
        return [encode_value(x) for x in v]
    if isinstance(v, dict):
        return {k: encode_value(x) for k, x in v.items()}
    if isinstance(v, float) and not math.isfinite(v):
        return {"__float__": repr(v)}
    return v


def decode_value(v: Any) -> Any:
    if isinstance(v, dict):
        if set(v) == {"__tuple__"}:
            return tuple(decode_value(x) for x in v["__tuple__"])
        if set(v) == {"__float__"}:
            return float(v["__float__"])
        return {k: decode_value(x) for k, x in v.items()}
    if isinstance(v, list):
        return [decode_value(x) for x in v]
    return v


# an intent record as the list of its values in this order (the fixture holds a few hundred of them)
INTENT_FIELDS = ("target_duration_s", "segments", "alignment", "alignment_raw", "lyrics", "profile")


ALIGNMENT_FIELDS = tuple(f"phrase_boundary.weights.{k}" for k in ("acoustic_pause", "asr_gap", "sentence_end", "beat_affinity", "mdd_affinity",
                                                                  "breath", "inside_word_penalty", "singing_penalty")) + (
    "vpbd.beat_candidates.base_score", "global_planner.beat_conflict_weight")


def pack_alignment(overrides: Dict[str, Any]) -> List[Any]:
    """`derive_alignment_overrides`' map as its values in `ALIGNMENT_FIELDS` order; the empty map as []."""
    assert not overrides or set(overrides) == set(ALIGNMENT_FIELDS), sorted(overrides)
    return [overrides[k] for k in ALIGNMENT_FIELDS] if overrides else []


def pack_intent(intent: Dict[str, Any]) -> List[Any]:
    assert tuple(intent) == INTENT_FIELDS, tuple(intent)
    return [intent[k] for k in INTENT_FIELDS]


# Two ways the fixture avoids holding the same thing many times.  `applied_overrides` of every AutoProfile record is the same list
# of keys (the profile's and the eight weights): held once, a mark in its place.  The run with unmarked keys is held as what
# differs from the run with marked keys, dict fields one level down.
APPLIED_MARK = "auto_applied_overrides"
_MISSING = object()


def fold_applied(meta: Any, keys: List[str]) -> Any:
    if isinstance(meta, dict) and meta.get("applied_overrides") == keys:
        return dict(meta, applied_overrides=APPLIED_MARK)
    return meta


def unfold_applied(meta: Any, keys: List[str]) -> Any:
    if isinstance(meta, dict) and meta.get("applied_overrides") == APPLIED_MARK:
        return dict(meta, applied_overrides=list(keys))
    return meta


def delta(base: Dict[str, Any], other: Dict[str, Any]) -> Dict[str, Any]:
    assert set(base) == set(other)
    out: Dict[str, Any] = {}
    for k, v in other.items():
        if v == base[k]:
            continue
        if isinstance(v, dict) and isinstance(base[k], dict):
            out[k] = {"set": {kk: vv for kk, vv in v.items() if base[k].get(kk, _MISSING) != vv}, "drop": [kk for kk in base[k] if kk not in v]}
        else:
            out[k] = {"is": v}
    return out


def patch(base: Dict[str, Any], changes: Dict[str, Any]) -> Dict[str, Any]:
    out = dict(base)
    for k, c in changes.items():
        out[k] = c["is"] if "is" in c else {**{kk: vv for kk, vv in base[k].items() if kk not in c["drop"]}, **c["set"]}
    return out


def expected_run(row: Dict[str, Any], marked: bool, keys: List[str]) -> Dict[str, Any]:
    """The recorded run of a runtime case (`row`: its `marked` record and `unmarked` changes) as it was before folding."""
    rec = row["marked"] if marked or row["unmarked"] == "same_as_marked" else patch(row["marked"], row["unmarked"])
    return dict(rec, meta=unfold_applied(rec["meta"], keys))


# ---- signals for the coverage kernel ---------------------------------------------------------------------------------------------
def _ulp_below(v: np.float32) -> np.float32:
    return np.nextafter(F32(v), F32(0.0))


def _ulp_above(v: np.float32) -> np.float32:
    return np.nextafter(F32(v), F32(np.inf))


def _place(x: np.ndarray, values, rng) -> None:
    """`values` at distinct seeded positions, as many as fit (the first of them first)."""
    k = min(len(values), x.size)
    pos = rng.permutation(x.size)[:k]
    x[pos] = np.asarray(values[:k], dtype=F32)


def rounds_down_peak(rng) -> np.float32:
    """A float32 peak p in [0.1, 1) whose float32 threshold float32(p * 0.03) lies BELOW the float64 product."""
    while True:
        p = F32(rng.uniform(0.1, 1.0))
        if float(F32(float(p) * 0.03)) < float(p) * 0.03:
            return p


def coverage_signal(recipe: str, n: int, seed: int) -> np.ndarray:
    """float32 [n] by recipe name; every recipe is defined for every n >= 1 (special samples are placed as far as they fit)."""
    rng = np.random.default_rng([seed, n])
    if recipe == "noise_half":                  # about half the samples far below 3 % of the peak
        x = (rng.standard_normal(n) * 0.3).astype(F32)
        x[rng.random(n) < 0.5] *= F32(0.004)
        return x
    if recipe == "zeros":
        return np.zeros(n, dtype=F32)
    if recipe in ("peak_5e-10", "peak_2e-9"):   # coverage 0.0 by the 1e-9 rule / the floor 1e-5 above every sample
        peak = F32(5e-10 if recipe == "peak_5e-10" else 2e-9)
        x = (rng.uniform(-0.9, 0.9, n)).astype(F32) * peak
        _place(x, [peak], rng)
        return x
    if recipe == "floor_edges":                 # peak 1e-4: 3 % of it is 3e-6, the floor 1e-5 decides; samples on it and one ulp off
        x = rng.uniform(-2e-5, 2e-5, n).astype(F32)
        at = F32(1e-5)
        _place(x, [F32(1e-4), at, _ulp_below(at), _ulp_above(at), -at, -_ulp_below(at)], rng)
        return x
    if recipe == "thr_rounds_down":             # a sample equal to the float32 threshold, which lies below peak * 0.03 in float64
        p = rounds_down_peak(rng)
        thr = F32(float(p) * 0.03)
        x = rng.uniform(-1.5, 1.5, n).astype(F32) * thr
        _place(x, [p, thr, -thr, _ulp_below(thr), _ulp_above(thr)], rng)
        return x
    if recipe == "negative_peak":
        x = (rng.standard_normal(n) * 0.2).astype(F32)
        x[rng.random(n) < 0.4] *= F32(0.01)
        _place(x, [-(np.max(np.abs(x)) * F32(1.5) + F32(0.25))], rng)
        return x
    if recipe == "zeros_denormals":             # -0.0, +0.0 and denormals only: peak far below 1e-9
        pool = np.array([-0.0, 0.0, 1e-40, -3e-42, 1.4e-45, -1.1e-38], dtype=F32)
        return pool[rng.integers(0, pool.size, n)]
    if recipe == "signal_with_denormals":       # a normal signal whose quiet half is -0.0 and denormals
        x = (rng.standard_normal(n) * 0.25).astype(F32)
        quiet = rng.random(n) < 0.5
        pool = np.array([-0.0, 1e-40, -3e-42, 1.4e-45], dtype=F32)
        x[quiet] = pool[rng.integers(0, pool.size, int(quiet.sum()))]
        return x
    if recipe in ("peak_last", "peak_first"):
        x = (rng.standard_normal(n) * 0.1).astype(F32)
        x[rng.random(n) < 0.5] *= F32(0.01)
        x[-1 if recipe == "peak_last" else 0] = F32(0.875)
        return x
    raise KeyError(recipe)


SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
EDGE_RECIPES = ("zeros", "peak_5e-10", "peak_2e-9", "floor_edges", "thr_rounds_down", "negative_peak", "zeros_denormals",
                "signal_with_denormals", "peak_last", "peak_first")


def coverage_cases(grid_samples: int) -> List[Tuple[str, int, int]]:
    """(recipe, n, seed): the noise at every small size and at 2 * grid_samples + 5 (`grid_samples`: what one step of the kernel's
    largest grid covers, `_native.PROFILE_GRID_SAMPLES`), the edge recipes at sizes around one wave, one workgroup tile and four."""
    cases = [("noise_half", n, 11) for n in SMALL_SIZES] + [("noise_half", 2 * grid_samples + 5, 12)]
    for i, recipe in enumerate(EDGE_RECIPES):
        cases += [(recipe, n, 20 + i) for n in (1, 65, 257, 4097)]
    return cases


# ---- caches for `estimate_style` -------------------------------------------------------------------------------------------------
def style_cache(spec: Dict[str, Any]) -> types.SimpleNamespace:
    """A cache-like object from a spec of `STYLE_CASES`: `main_bpm` (None: no `bpm_features`), `global_mdd`, `rms`, `coverage`
    (None: the attribute is absent), `beat_times` (a list; None: absent)."""
    cache = types.SimpleNamespace(global_mdd=spec["global_mdd"], rms_series=np.asarray(spec["rms"], dtype=F32))
    cache.bpm_features = None if spec.get("main_bpm") is None else types.SimpleNamespace(main_bpm=spec["main_bpm"])
    if spec.get("coverage") is not None:
        cache.vocal_coverage_ratio = spec["coverage"]
    if spec.get("beat_times") is not None:
        cache.beat_times = list(spec["beat_times"])
    return cache


_EVEN, _MID, _UNEVEN = [0.50, 0.55, 0.52, 0.49], [0.40, 0.52, 0.47], [0.10, 0.90, 0.20, 1.00]
STYLE_CASES: List[Dict[str, Any]] = [
    {"name": "ballad", "main_bpm": 80.0, "global_mdd": 0.30, "rms": _EVEN, "coverage": 0.70},
    {"name": "ballad_below_first_anchor", "main_bpm": 55.0, "global_mdd": 0.30, "rms": _EVEN, "coverage": 0.70},
    {"name": "edm", "main_bpm": 128.0, "global_mdd": 0.50, "rms": _UNEVEN, "coverage": 0.40},
    {"name": "rap_140_160", "main_bpm": 142.0, "global_mdd": 0.58, "rms": _MID, "coverage": 0.82},
    {"name": "rap_110_140", "main_bpm": 126.0, "global_mdd": 0.58, "rms": _MID, "coverage": 0.82},
    {"name": "rap_above_last_anchor", "main_bpm": 170.0, "global_mdd": 0.60, "rms": _MID, "coverage": 0.80},
    {"name": "pop_60_110", "main_bpm": 108.0, "global_mdd": 0.38, "rms": [0.2, 0.42, 0.31], "coverage": 0.56},
    {"name": "no_tempo_low_confidence", "main_bpm": 0.0, "global_mdd": 0.40, "rms": _MID, "coverage": 0.60},
    {"name": "tempo_from_beat_times", "main_bpm": None, "global_mdd": 0.50, "rms": _MID, "coverage": 0.75,
     "beat_times": [round(0.25 + 0.5 * i, 3) for i in range(24)]},
    # values that are meant to sit on a threshold (`on_threshold` names the comparisons)
    {"name": "on_bpm_88", "main_bpm": 88.0, "global_mdd": 0.30, "rms": _EVEN, "coverage": 0.70, "on_threshold": ["bpm:88"]},
    {"name": "on_anchor_110", "main_bpm": 110.0, "global_mdd": 0.30, "rms": _MID, "coverage": 0.60, "on_threshold": ["bpm:110"]},
]


# ---- runtime cases: a smart-cut configuration on a seeded track ---------------------------------------------------------------------
# `tempo` (None: the cache has no `bpm_features` and its beats, a list, give the tempo) and `global_mdd` complete `asr_case`'s cache;
# `coverage`: a ratio the cache already carries (the stem is then not looked at); `mute_tail`: that share of the stem's end is
# silenced (sparser vocals); `smart_cut`: the dotted keys of the run.  The last two give different results when their keys count
# as set by the caller and when they do not.
SMART_CUT_CASES: List[Dict[str, Any]] = [
    {"seed": 41, "tempo": 120.0, "global_mdd": 0.50, "smart_cut": {"smart_cut.segments": "many", "smart_cut.alignment": "beat_lean"}},
    {"seed": 43, "tempo": 150.0, "global_mdd": 0.60, "mute_tail": 0.25, "smart_cut": {"smart_cut.profile": "auto", "smart_cut.segments": "few"}},
    {"seed": 45, "tempo": 132.0, "global_mdd": 0.55, "smart_cut": {"smart_cut.profile": "rap", "smart_cut.alignment": "beat"}},
    {"seed": 48, "tempo": 130.0, "global_mdd": 0.60, "coverage": 0.90, "smart_cut": {"smart_cut.alignment": "balanced"}},
    {"seed": 49, "tempo": 96.0, "global_mdd": 0.42, "smart_cut": {"smart_cut.segments": "medium", "smart_cut.alignment": 0.5}},
    {"seed": 50, "tempo": 128.0, "global_mdd": 0.50,
     "smart_cut": {"smart_cut.segments": "many", "smart_cut.target_duration_s": [5.0, 12.0], "smart_cut.alignment": "lyric_lean"}},
]


def smart_cut_case(spec: Dict[str, Any]):
    """-> (cache, pauses, vocal, timeline payload) of `asr_case(spec["seed"])` with the cache completed from `spec`."""
    cache, pauses, vocal, payload = asr_case(spec["seed"])
    cache.global_mdd = spec["global_mdd"]
    if spec["tempo"] is None:
        cache.bpm_features = None
        cache.beat_times = [float(t) for t in cache.beat_times]
    else:
        cache.bpm_features = types.SimpleNamespace(main_bpm=spec["tempo"])
    if spec.get("coverage") is not None:
        cache.vocal_coverage_ratio = spec["coverage"]
    if spec.get("mute_tail"):
        vocal = vocal.copy()
        vocal[int(len(vocal) * (1.0 - spec["mute_tail"])):] = 0.0
    return cache, pauses, vocal, payload


__all__ = ["encode_value", "decode_value", "INTENT_FIELDS", "pack_intent", "ALIGNMENT_FIELDS", "pack_alignment", "APPLIED_MARK", "fold_applied", "unfold_applied", "delta", "patch", "expected_run", "coverage_signal", "coverage_cases", "rounds_down_peak", "SMALL_SIZES", "EDGE_RECIPES",
           "style_cache", "STYLE_CASES", "SMART_CUT_CASES", "smart_cut_case"]
