"""The smart-cut intent surface and AutoProfile: from what a caller asks for - how many segments (`few` / `medium` / `many` or
`(min_s, max_s)`), where cuts should lean (`lyric` ... `beat` or 0..1), which style profile (`auto` or a name) - to the dotted
runtime overrides the VPBD modes already read (`phrase_boundary.weights.*`, `vpbd.beat_candidates.base_score`, `global_planner.*`,
`segment_layout.soft_*`, `quality_control.*`, `pure_vocal_detection.*`).

This is the library's restatement of the reference's `src/audio_cut/config/auto_profile.py` (public names, return shapes, warnings,
error conditions and rounding kept) and of the part of `src/audio_cut/config/derive.py:149-268` behind `apply_profile_overrides`.
The four style profiles are a table here (`_PROFILE_SCHEMA`), as `config.DEFAULTS` is for `expert.yaml`; the values every function
returns are pinned by `tests/golden/auto_profile.json`, recorded from the reference's own functions.

Host code throughout: the inputs are four track-global numbers.  The one full-track computation behind them, the vocal coverage,
is `Context.vocal_coverage` (include/audiocut_hip_profile.h); `SeamlessSplitter._attach_vocal_coverage` puts it on the cache.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Any, Dict, Iterable, Mapping, Optional, Set, Tuple

import numpy as np

# ---- the stops of the two intent axes ---------------------------------------------------------------------------------------------
ALIGNMENT_STOPS: Dict[str, float] = {"lyric": 0.0, "lyric_lean": 0.25, "balanced": 0.5, "beat_lean": 0.75, "beat": 1.0}
SEGMENT_DURATION_STOPS: Dict[str, Tuple[float, float]] = {"few": (10.0, 18.0), "medium": (5.0, 12.0), "many": (3.0, 8.0)}
_MEDIUM = SEGMENT_DURATION_STOPS["medium"]

WEIGHT_KEYS = ("acoustic_pause", "asr_gap", "sentence_end", "beat_affinity", "mdd_affinity", "breath", "inside_word_penalty",
               "singing_penalty")


def _weights(*values: float) -> Dict[str, float]:
    return dict(zip(WEIGHT_KEYS, values))


# the ends of the alignment axis when the configuration gives none (`phrase_boundary.alignment_poles` carries the same numbers)
LYRIC_POLE = _weights(0.38, 0.26, 0.22, 0.02, 0.06, 0.10, 0.85, 0.50)
BEAT_POLE = _weights(0.22, 0.10, 0.08, 0.32, 0.12, 0.10, 0.80, 0.50)
# phrase-boundary weights per style
STYLE_WEIGHTS: Dict[str, Dict[str, float]] = {
    "ballad": _weights(0.40, 0.20, 0.20, 0.05, 0.05, 0.10, 0.80, 0.50),
    "pop": _weights(0.35, 0.20, 0.15, 0.08, 0.10, 0.12, 0.80, 0.50),
    "rap": _weights(0.28, 0.16, 0.12, 0.14, 0.14, 0.16, 0.85, 0.50),
    "edm": _weights(0.25, 0.12, 0.10, 0.22, 0.14, 0.17, 0.85, 0.50),
}
# tempo anchors AutoProfile interpolates the profile overrides between
PROFILE_ANCHORS = ((60.0, "ballad"), (110.0, "pop"), (140.0, "rap"), (160.0, "edm"))

# ---- the style profiles: the eleven schema knobs, defaults first, then what each profile changes ----------------------------------
_SCHEMA_DEFAULT = {"name": "default", "comment": "Minimal configuration for Vocal Smart Splitter schema v3.",
                   "sample_rate": 44100, "channels": 1, "min_pause_s": 0.5, "min_gap_s": 1.0, "guard_max_shift_ms": 150.0,
                   "guard_floor_db": -60.0, "base_ratio": 0.26, "bpm_strength": 0.4, "mdd_strength": 0.2, "nms_topk": 4}
_PROFILE_SCHEMA: Dict[str, Dict[str, Any]] = {
    "ballad": {"min_pause_s": 0.6, "min_gap_s": 1.2, "base_ratio": 0.24, "bpm_strength": 0.3, "guard_max_shift_ms": 220.0},
    "pop": {"base_ratio": 0.26, "bpm_strength": 0.45, "guard_max_shift_ms": 160.0, "nms_topk": 4},
    "rap": {"min_pause_s": 0.38, "base_ratio": 0.25, "bpm_strength": 0.7, "mdd_strength": 0.45, "guard_floor_db": -62.0, "nms_topk": 5},
    "edm": {"min_pause_s": 0.4, "base_ratio": 0.22, "bpm_strength": 0.8, "mdd_strength": 0.35, "nms_topk": 6},
}
PROFILE_NAMES = tuple(_PROFILE_SCHEMA)


def _clip(v: float, lo: float, hi: float) -> float:
    return max(lo, min(hi, v))


def _schema_override_map(schema: Mapping[str, Any]) -> Dict[str, Any]:
    """`build_runtime_override_map` (`derive.py:149-245`): the flat runtime overrides of one set of schema knobs."""
    bpm_strength = _clip(float(schema["bpm_strength"]), 0.0, 1.5)
    spread = 0.08 * bpm_strength                                    # `_derive_bpm_multipliers`
    slow, medium, fast = round(1.0 + spread, 4), 1.0, round(1.0 - spread, 4)
    span = 0.15 + 0.05 * bpm_strength                               # `_derive_bpm_clamp`
    base_ratio = float(schema["base_ratio"])
    pvd, rta, qc = "pure_vocal_detection.", "pure_vocal_detection.relative_threshold_adaptation.", "quality_control."
    flat = {
        "meta.schema_version": 3, "meta.schema_name": schema["name"], "meta.schema_comment": schema["comment"],
        "audio.sample_rate": int(schema["sample_rate"]), "audio.channels": int(schema["channels"]),
        pvd + "min_pause_duration": float(schema["min_pause_s"]),
        pvd + "peak_relative_threshold_ratio": base_ratio,
        pvd + "rms_relative_threshold_ratio": _clip(base_ratio + 0.06, 0.05, 0.7),          # `_derive_rms_ratio`
        rta + "enable": True,
        rta + "bpm.slow_multiplier": slow, rta + "bpm.medium_multiplier": medium, rta + "bpm.fast_multiplier": fast,
        rta + "pause_stats_multipliers.slow": slow, rta + "pause_stats_multipliers.medium": medium,
        rta + "pause_stats_multipliers.fast": fast,
        rta + "mdd.base": 1.0, rta + "mdd.gain": round(0.2 * _clip(float(schema["mdd_strength"]), 0.0, 2.0), 4),   # `_derive_mdd_params`
        rta + "clamp_min": round(1.0 - span, 4), rta + "clamp_max": round(1.0 + span, 4),
        pvd + "valley_scoring.max_kept_after_nms": max(60, int(schema["nms_topk"]) * 20),  # `_derive_topk_cap`
        qc + "min_split_gap": float(schema["min_gap_s"]), qc + "nms_topk_per_10s": int(schema["nms_topk"]),
        qc + "enforce_quiet_cut.search_right_ms": float(schema["guard_max_shift_ms"]),
        qc + "enforce_quiet_cut.floor_db_override": float(schema["guard_floor_db"]),
    }
    return {k: v for k, v in flat.items() if v is not None}


def default_schema_overrides() -> Dict[str, Any]:
    """The override map of the schema defaults alone (no profile)."""
    return _schema_override_map(_SCHEMA_DEFAULT)


def apply_profile_overrides(name: str) -> Dict[str, Any]:
    """The flat runtime override map of style profile `name` (`ballad` / `pop` / `rap` / `edm`): its knobs over the schema
    defaults, derived, plus `meta.profile`.  25 keys; `audio.*` and `meta.*` are among them as in the reference."""
    if name not in _PROFILE_SCHEMA:
        raise KeyError(f"profile {name!r} not found. available={sorted(_PROFILE_SCHEMA)}")
    flat = _schema_override_map({**_SCHEMA_DEFAULT, **_PROFILE_SCHEMA[name]})
    flat.setdefault("meta.profile", name)
    return flat


# ---- intent resolution -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class StyleEstimate:
    """What `estimate_style` concludes from a feature cache: the nearest profile, how sure, and the four features it read."""
    profile: str
    confidence: float
    features: Dict[str, float]
    fallback_reason: Optional[str] = None


def _unit(v: float) -> float:
    return _clip(v, 0.0, 1.0)


def resolve_alignment(value: Any) -> float:
    """A stop name, a number or a numeric string -> the alignment in [0, 1] (clamped, 4 decimals); nothing -> 0.5."""
    if value is None or value == "":
        return 0.5
    if isinstance(value, str):
        name = value.strip().lower()
        if not name:
            return 0.5
        if name in ALIGNMENT_STOPS:
            return ALIGNMENT_STOPS[name]
        try:
            number = float(name)
        except ValueError as exc:
            raise ValueError(f"smart_cut.alignment must be one of {', '.join(sorted(ALIGNMENT_STOPS))} "
                             f"or a float between 0.0 and 1.0") from exc
    else:
        try:
            number = float(value)
        except (TypeError, ValueError) as exc:
            raise ValueError("smart_cut.alignment must be a stop name or numeric value") from exc
    if not math.isfinite(number):
        raise ValueError("smart_cut.alignment must be finite")
    return round(_unit(number), 4)


def _checked_range(lo: Any, hi: Any) -> Tuple[float, float]:
    lo, hi = float(lo), float(hi)
    if lo <= 0.0 or hi <= lo:
        raise ValueError("smart_cut.target_duration_s must be increasing positive seconds")
    return lo, hi


def resolve_segment_duration(value: Any) -> Tuple[float, float]:
    """A density stop, `"MIN-MAX"` or a pair -> (min_s, max_s); nothing -> the `medium` stop."""
    if value is None or value == "":
        return _MEDIUM
    if isinstance(value, str):
        name = value.strip().lower()
        if name in SEGMENT_DURATION_STOPS:
            return SEGMENT_DURATION_STOPS[name]
        if "-" in name:
            return _checked_range(*name.split("-", 1))
        raise ValueError("smart_cut.segments must be few, medium, many, or MIN-MAX seconds")
    if isinstance(value, (list, tuple)) and len(value) == 2:
        return _checked_range(value[0], value[1])
    raise ValueError("smart_cut.segments must be few, medium, many, or [min_s, max_s]")


def _rounded(pair: Iterable[float]) -> Tuple[float, ...]:
    return tuple(round(v, 4) for v in pair)


def _blank(value: Any) -> bool:
    return value is None or (isinstance(value, str) and value.strip() == "")


def _is_medium(value: Any) -> bool:
    try:
        return _rounded(resolve_segment_duration(value)) == _rounded(_MEDIUM)
    except Exception:
        return False


# A value counts as stated when it is none of the defaults.  The test is set membership, as in the reference: an unhashable value
# (a list) is a TypeError there and here - pairs are passed as tuples.
_ALIGNMENT_DEFAULTS = frozenset({None, "", "balanced", 0.5})
_SEGMENTS_DEFAULTS = frozenset({None, "", "medium"})


def _target_duration(smart_cut: Mapping[str, Any], explicit: Set[str], *, warn_level: int) -> Tuple[float, float]:
    """`segments` against `target_duration_s`: the numeric pair wins when it is explicit (set by the caller, or not the default)
    and differs; `segments` wins when only it is explicit; otherwise the pair stands."""
    seg_raw, tgt_raw = smart_cut.get("segments", None), smart_cut.get("target_duration_s", None)
    by_segments = resolve_segment_duration(seg_raw)
    if tgt_raw is None:
        return by_segments
    target = resolve_segment_duration(tgt_raw)
    target_stated = "smart_cut.target_duration_s" in explicit or target != _MEDIUM
    segments_stated = "smart_cut.segments" in explicit or seg_raw not in _SEGMENTS_DEFAULTS
    if target != by_segments:
        if target_stated:
            if segments_stated:
                warnings.warn("smart_cut.target_duration_s is explicit and wins over smart_cut.segments", UserWarning,
                              stacklevel=warn_level)
            return target
        if segments_stated:
            return by_segments
    return target


def resolve_smart_cut_intent(smart_cut: Mapping[str, Any], *, explicit_keys: Optional[Set[str]] = None) -> Dict[str, Any]:
    """The `smart_cut` section -> machine values: `target_duration_s`, the `segments` stop it equals (or None), `alignment` in
    [0, 1] and as given, `lyrics`, `profile`.  `explicit_keys`: the dotted keys the caller set on purpose
    (`config.get_runtime_override_keys`).  The deprecated `cut_style` warns and maps `rhythmic` to alignment 0.7 and `dense` to
    `many`, unless the axis it would set was stated."""
    explicit = explicit_keys or set()
    text = lambda key, default: str(smart_cut.get(key, default) or default).strip().lower()
    profile, lyrics, cut_style = text("profile", "auto"), text("lyrics", "auto"), str(smart_cut.get("cut_style", "") or "").strip().lower()
    align_raw, seg_raw, tgt_raw = (smart_cut.get(k, None) for k in ("alignment", "segments", "target_duration_s"))

    align_stated = "smart_cut.alignment" in explicit or align_raw not in _ALIGNMENT_DEFAULTS
    target_default = _blank(tgt_raw) or _is_medium(tgt_raw)
    seg_stated = "smart_cut.segments" in explicit or seg_raw not in _SEGMENTS_DEFAULTS

    if cut_style and cut_style != "natural":
        warnings.warn("smart_cut.cut_style is deprecated; use smart_cut.alignment and smart_cut.segments instead",
                      DeprecationWarning, stacklevel=2)
        if align_stated and cut_style == "rhythmic":
            warnings.warn("smart_cut.alignment is explicit, so deprecated cut_style alignment mapping is ignored",
                          DeprecationWarning, stacklevel=2)
        elif cut_style == "rhythmic":
            align_raw = 0.7
        if cut_style == "dense" and not seg_stated and target_default:
            seg_raw = "many"

    alignment = resolve_alignment(align_raw)
    resolved = dict(smart_cut)
    if align_raw is not None:
        resolved["alignment"] = align_raw
    if seg_raw is not None:
        resolved["segments"] = seg_raw
    target = _target_duration(resolved, explicit, warn_level=3)

    stop = seg_raw.strip().lower() if isinstance(seg_raw, str) else None
    if stop not in SEGMENT_DURATION_STOPS:
        stop = next((name for name, pair in SEGMENT_DURATION_STOPS.items() if _rounded(pair) == _rounded(target)), None)
    return {"target_duration_s": [round(target[0], 4), round(target[1], 4)], "segments": stop, "alignment": alignment,
            "alignment_raw": align_raw if align_raw is not None else "balanced", "lyrics": lyrics, "profile": profile}


def should_apply_duration_overrides(smart_cut: Mapping[str, Any], *, explicit_keys: Optional[Set[str]] = None) -> bool:
    """Whether the intent moves the planner's duration knobs: a stated `segments` or `target_duration_s`, or either off its default."""
    explicit = explicit_keys or set()
    if "smart_cut.segments" in explicit or "smart_cut.target_duration_s" in explicit:
        return True
    if smart_cut.get("segments", None) not in _SEGMENTS_DEFAULTS:
        return True
    target = smart_cut.get("target_duration_s", None)
    return not _blank(target) and not _is_medium(target)


def derive_smart_cut_overrides(smart_cut: Mapping[str, Any], *, explicit_keys: Optional[Set[str]] = None) -> Dict[str, float]:
    """Planner, layout and quality-control duration knobs of the resolved target range: hard limits at 0.4 x min (at least 1 s)
    and 1.5 x max."""
    lo, hi = _target_duration(smart_cut, explicit_keys or set(), warn_level=3)
    lo4, hi4 = round(lo, 4), round(hi, 4)
    hard_lo, hard_hi = round(max(1.0, lo * 0.4), 4), round(hi * 1.5, 4)
    return {"global_planner.target_min_s": lo4, "global_planner.target_max_s": hi4, "global_planner.hard_min_s": hard_lo,
            "global_planner.hard_max_s": hard_hi, "segment_layout.soft_min_s": lo4, "segment_layout.soft_max_s": hi4,
            "quality_control.segment_max_duration": hard_hi}


# ---- the alignment axis ----------------------------------------------------------------------------------------------------------
def _poles(alignment_poles: Optional[Mapping[str, Any]]) -> Tuple[Dict[str, float], Dict[str, float]]:
    lyric, beat = dict(LYRIC_POLE), dict(BEAT_POLE)
    if isinstance(alignment_poles, Mapping):
        for pole, given in ((lyric, alignment_poles.get("lyric", {})), (beat, alignment_poles.get("beat", {}))):
            if isinstance(given, Mapping):
                pole.update({k: float(given[k]) for k in WEIGHT_KEYS if k in given})
    return lyric, beat


def _mix(a: float, b: float, t: float) -> float:
    return float(a) + (float(b) - float(a)) * float(t)


def _beat_base_score(a: float) -> float:
    """Score of the beat candidates along the axis: none up to 0.3, rising to 0.3 at the middle and 0.65 at the beat end."""
    if a <= 0.3:
        return 0.0
    if a <= 0.5:
        return 0.3 * ((a - 0.3) / 0.2)
    return 0.3 + (0.65 - 0.3) * ((a - 0.5) / 0.5)


def derive_alignment_overrides(alignment: Any, style_weights: Mapping[str, Any], *,
                               alignment_poles: Optional[Mapping[str, Any]] = None) -> Dict[str, Any]:
    """Phrase-boundary weights, beat-candidate score and beat-conflict weight of an alignment: the style's weights blended
    towards the lyric pole below 0.5 and the beat pole above it.  Exactly balanced: nothing.  `style_weights` may carry bare
    or `phrase_boundary.weights.`-prefixed keys; a missing weight takes the `pop` value."""
    a = resolve_alignment(alignment)
    if abs(a - 0.5) <= 1e-9:
        return {}
    lyric, beat = _poles(alignment_poles)

    def style(key: str) -> float:
        for name in (key, f"phrase_boundary.weights.{key}"):
            if name in style_weights:
                return float(style_weights[name])
        return float(STYLE_WEIGHTS["pop"].get(key, 0.0))

    if a <= 0.5:
        blend = {k: _mix(lyric[k], style(k), a * 2.0) for k in WEIGHT_KEYS}
    else:
        blend = {k: _mix(style(k), beat[k], (a - 0.5) * 2.0) for k in WEIGHT_KEYS}
    out: Dict[str, Any] = {f"phrase_boundary.weights.{k}": round(v, 4) for k, v in blend.items()}
    out["vpbd.beat_candidates.base_score"] = round(_beat_base_score(a), 4)
    out["global_planner.beat_conflict_weight"] = round(0.30 * a, 4)
    return out


# ---- AutoProfile -----------------------------------------------------------------------------------------------------------------
def _tempo_from_beats(beat_times: Any) -> float:
    beats = np.asarray([] if beat_times is None else list(beat_times), dtype=np.float32)
    if beats.size < 2:
        return 0.0
    steps = np.diff(beats)
    steps = steps[steps > 1e-6]
    return 60.0 / float(np.median(steps)) if steps.size else 0.0


def _track_features(cache: Any) -> Dict[str, float]:
    """bpm (the cache's main BPM, else the median beat interval's), global MDD, the coefficient of variation of the float32 RMS
    series, and the vocal coverage, each rounded to 4 decimals."""
    bpm = float(getattr(getattr(cache, "bpm_features", None), "main_bpm", 0.0) or 0.0)
    if bpm <= 0.0:
        bpm = _tempo_from_beats(getattr(cache, "beat_times", []))
    rms = np.asarray(getattr(cache, "rms_series", []), dtype=np.float32)
    mean = float(np.mean(rms)) if rms.size else 0.0
    energy_cv = float(np.std(rms) / max(mean, 1e-9)) if mean > 0.0 else 0.0
    return {"bpm": round(max(0.0, bpm), 4),
            "global_mdd": round(_unit(float(getattr(cache, "global_mdd", 0.0) or 0.0)), 4),
            "energy_cv": round(max(0.0, energy_cv), 4),
            "vocal_coverage_ratio": round(_unit(float(getattr(cache, "vocal_coverage_ratio", 0.0) or 0.0)), 4)}


def estimate_style(cache: Any) -> StyleEstimate:
    """Rule-based style of a track from its cache: slow and even -> ballad; fast, uneven, sparse vocals -> edm; fast, dense,
    vocals nearly throughout -> rap; else pop.  No tempo: pop at low confidence."""
    f = _track_features(cache)
    bpm, mdd, cv, cover = f["bpm"], f["global_mdd"], f["energy_cv"], f["vocal_coverage_ratio"]
    if bpm <= 0.0:
        return StyleEstimate("pop", 0.25, f, "low_confidence")
    if bpm <= 88.0 and cv <= 0.25:
        return StyleEstimate("ballad", 0.78, f)
    if bpm >= 122.0 and cv >= 0.65 and cover <= 0.55:
        return StyleEstimate("edm", 0.82, f)
    if bpm >= 118.0 and mdd >= 0.45 and cover >= 0.68:
        return StyleEstimate("rap", 0.82, f)
    return StyleEstimate("pop", 0.70, f)


def _anchor_weights(estimate: StyleEstimate) -> Dict[str, float]:
    """Profile weights by tempo: one profile outside the anchors (and for edm), else the two neighbours, linearly."""
    bpm = float(estimate.features.get("bpm", 0.0) or 0.0)
    if estimate.profile == "edm":
        return {"edm": 1.0}
    if bpm <= PROFILE_ANCHORS[0][0]:
        return {PROFILE_ANCHORS[0][1]: 1.0}
    for (lo_bpm, lo_name), (hi_bpm, hi_name) in zip(PROFILE_ANCHORS, PROFILE_ANCHORS[1:]):
        if lo_bpm <= bpm <= hi_bpm:
            hi_w = (bpm - lo_bpm) / max(hi_bpm - lo_bpm, 1e-9)
            kept = {k: round(float(v), 4) for k, v in ((lo_name, 1.0 - hi_w), (hi_name, hi_w)) if float(v) > 1e-6}
            total = sum(kept.values())
            return {k: round(v / total, 4) for k, v in kept.items()} if total > 0.0 else {"pop": 1.0}
    return {PROFILE_ANCHORS[-1][1]: 1.0}


def _blend_profiles(anchor_weights: Mapping[str, float]) -> Dict[str, Any]:
    """The weighted mean (6 decimals) of the anchors' override maps where every anchor's value is a number - booleans and
    integers included, which therefore come out as floats - else the heaviest anchor's value."""
    maps = {name: apply_profile_overrides(name) for name, w in anchor_weights.items() if w > 0.0}
    heaviest = max(anchor_weights.items(), key=lambda kv: kv[1])[0]
    out: Dict[str, Any] = {}
    for key in sorted({k for m in maps.values() for k in m}):
        values = [maps[name].get(key) for name in anchor_weights if name in maps]
        if values and all(isinstance(v, (int, float)) for v in values):
            out[key] = round(sum(float(maps[name][key]) * float(anchor_weights[name]) for name in anchor_weights if name in maps), 6)
        elif key in maps[heaviest]:
            out[key] = maps[heaviest][key]
    return out


def build_style_weight_overrides(profile: str, *, cut_style: str = "natural") -> Dict[str, float]:
    """`phrase_boundary.weights.*` of a style (an unknown one: pop), with the deprecated `cut_style` nudges."""
    w = dict(STYLE_WEIGHTS.get(profile, STYLE_WEIGHTS["pop"]))
    if cut_style == "rhythmic":
        w["beat_affinity"] = min(0.25, w["beat_affinity"] + 0.04)
        w["breath"] = min(0.20, w["breath"] + 0.02)
        w["acoustic_pause"] = max(0.20, w["acoustic_pause"] - 0.04)
    elif cut_style == "dense":
        w["breath"] = min(0.22, w["breath"] + 0.04)
        w["sentence_end"] = max(0.08, w["sentence_end"] - 0.02)
    return {f"phrase_boundary.weights.{k}": round(v, 4) for k, v in w.items()}


def build_auto_profile_overrides(estimate: StyleEstimate, *, cut_style: str = "natural") -> Dict[str, Any]:
    """The runtime overrides of an estimate - the anchors' profile maps blended by tempo, the style's phrase weights - and the
    `meta.auto_profile` record of what was decided.  Below confidence 0.6 everything is pop."""
    sure = estimate.confidence >= 0.6
    anchors = _anchor_weights(estimate) if sure else {"pop": 1.0}
    style = estimate.profile if sure else "pop"
    out = _blend_profiles(anchors)
    out.update(build_style_weight_overrides(style, cut_style=cut_style))
    r4 = lambda v: None if v is None else round(float(v), 4)
    applied = sorted(k for k in out if not k.startswith("meta."))
    out["meta.auto_profile"] = {
        "style": style, "confidence": round(float(estimate.confidence), 4), "bpm": r4(estimate.features.get("bpm")),
        "mdd": r4(estimate.features.get("global_mdd")), "features": {k: r4(v) for k, v in estimate.features.items()},
        "anchor_weights": anchors, "fallback_reason": estimate.fallback_reason, "applied_overrides": applied}
    out["meta.profile"] = "auto"
    return out


__all__ = ["ALIGNMENT_STOPS", "SEGMENT_DURATION_STOPS", "StyleEstimate", "apply_profile_overrides", "build_auto_profile_overrides",
           "build_style_weight_overrides", "default_schema_overrides", "derive_alignment_overrides", "derive_smart_cut_overrides",
           "estimate_style", "resolve_alignment", "resolve_segment_duration", "resolve_smart_cut_intent",
           "should_apply_duration_overrides"]
