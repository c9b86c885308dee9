"""Hot-path configuration: the effective values of the reference's `config/expert.yaml` merged under
`config/unified.yaml` (what `get_config` returns there, `src/vocal_smart_splitter/utils/config_manager.py:485-495`),
restricted to the keys SURVEY.md Appendix A lists for the separate+detect path.

`get_config(path, default)` has the reference's semantics: dotted lookup, `default` when the key is absent
(several call sites rely on their literal default because the YAML omits the key).  `set_runtime_config`
/ `reset_runtime_config` mirror `config_manager.py:497-509` (dotted-key overrides layered on top), and
`get_runtime_override_keys` (`:512-515`) names the keys a caller set through it: the smart-cut intent layer
(`config/auto_profile.py`) treats those as stated on purpose even where the value equals the default.
"""
from __future__ import annotations

import copy
import os
from typing import Any, Dict, Set

DEFAULTS: Dict[str, Any] = {
    # the v2.8 intent surface (`unified.yaml:8-14`); read by `SeamlessSplitter._apply_smart_cut_runtime` alone
    "smart_cut": {"segments": "medium", "alignment": "balanced", "profile": "auto", "cut_style": "natural",
                  "target_duration_s": [5.0, 12.0], "lyrics": "auto"},
    # `gpu_decode`: .wav input is decoded on the device from the file's own bytes (`api.load_audio_device`); false: on the host
    "audio": {"sample_rate": 44100, "channels": 1, "gpu_decode": True},
    # the export format (`unified.yaml:49-51`): `wav` alone is written here; subtype: PCM_U8, PCM_16, PCM_24, PCM_32, FLOAT or DOUBLE
    "output": {"format": "wav", "wav": {"subtype": "PCM_24"}},
    "gpu_pipeline": {
        "enable": True, "prefer_device": "cuda", "strict_gpu": False,
        "chunk_seconds": 10.0, "overlap_seconds": 2.5, "halo_seconds": 0.5, "align_hop": 4096,
        "use_cuda_streams": True, "prefetch_pinned_buffers": 2, "inflight_chunks_limit": 2,
    },
    "enhanced_separation": {
        "backend": "mdx23", "enable_fallback": True,
        "mdx23": {"model_filename": "Kim_Vocal_1.onnx", "output_type": "auto"},
    },
    "analysis": {"features_cache": {"device": "auto"}},
    "musical_dynamic_density": {
        "energy_weight": 0.5, "spectral_weight": 0.3, "onset_weight": 0.2,
        "threshold_multiplier": 0.2, "max_multiplier": 1.4, "min_multiplier": 0.6,
    },
    "advanced_vad": {
        "focus_window_pad_s": 0.2, "focus_window_min_width_s": 0.0, "silero_merge_gap_ms": 120.0,
        "focus_merge_gap_s": 0.12, "silero_length_bucket": 4096,
    },
    "pure_vocal_detection": {
        "enable": True, "min_pause_duration": 0.5, "breath_duration_range": [0.1, 0.3],
        "f0_weight": 0.3, "formant_weight": 0.25, "spectral_weight": 0.25, "duration_weight": 0.2,
        "enable_relative_energy_mode": True,
        "peak_relative_threshold_ratio": 0.26, "rms_relative_threshold_ratio": 0.3,
        "relative_threshold_adaptation": {
            "enable": True, "clamp_min": 0.85, "clamp_max": 1.15,
            "bpm": {"slow_multiplier": 1.08, "medium_multiplier": 1.0, "fast_multiplier": 0.92},
            "mdd": {"base": 1.0, "gain": 0.2},
            "pause_stats_multipliers": {"slow": 1.08, "medium": 1.0, "fast": 0.92},
        },
        "pause_stats_adaptation": {
            "enable": True, "delta_db": 3.0, "morph_close_ms": 150, "morph_open_ms": 50,
            "sing_block_min_s": 2.0, "interlude_min_s": 4.0,
            "classify_thresholds": {
                "slow": {"mpd": 0.6, "p95": 1.2, "rr": 0.35},
                "fast": {"mpd": 0.25, "pr": 18, "rr": 0.15},
            },
        },
        "valley_scoring": {
            "w_len": 0.7, "w_quiet": 0.3, "w_flat": 0.5, "use_weighted_nms": True,
            "merge_close_ms": 450, "max_raw_candidates": 1200, "max_kept_after_nms": 200,
        },
    },
    "vocal_pause_splitting": {
        "local_rms_window_ms": 25, "silence_floor_percentile": 5, "silence_floor_allowance": 0.0,
        "lookahead_guard_ms": 120, "head_offset": 0.0, "tail_offset": 0.0, "voice_threshold": 0.5,
    },
    "quality_control": {
        "min_split_gap": 1.2, "segment_min_duration": 2.0, "segment_max_duration": 18.0,
        "pure_music_min_duration": 6.0, "segment_vocal_threshold_db": -50.0, "segment_min_mix_piece": 2.0,
        "local_boundary_refine": {"enable": True, "search_radius_ms": 500, "window_ms": 5, "min_drop_db": 5.0},
        "enforce_quiet_cut": {
            "enable": True, "win_ms": 80, "guard_db": 1.5, "search_right_ms": 450,
            "floor_percentile": 0.5, "floor_db_override": None,
        },
        # segment finishing (utils/segment_finish.py; `expert.yaml:105-107` and the literals of `AudioProcessor.normalize_audio`):
        # at these defaults the export is what it is without the feature
        "fade_in_duration": 0.0, "fade_out_duration": 0.0, "normalize_audio": False,
        "normalize_target_db": -20.0, "normalize_max_gain": 10.0,
    },
    "segment_layout": {"enable": True, "micro_merge_s": 2.0, "soft_min_s": 5.0, "soft_max_s": 12.0, "min_gap_s": 1.0, "beat_snap_ms": 50},
    "vpbd": {
        "enabled": True, "candidate_pool": "unified", "candidate_debug_json": True, "breath_score_scale": 0.6,
        "beat_candidates": {"enable": True, "bars_per_cut": 2, "base_score": 0.3},
    },
    "lyrics_alignment": {"enabled": False, "provider": "disabled", "strict": False},
    "phrase_boundary": {
        "word_edge_tolerance_ms": 60.0,
        "weights": {"acoustic_pause": 0.35, "asr_gap": 0.2, "sentence_end": 0.15, "beat_affinity": 0.08, "mdd_affinity": 0.1,
                    "breath": 0.12, "inside_word_penalty": 0.8, "singing_penalty": 0.5},
        # the two ends of the alignment axis (`expert.yaml:194-212`); `derive_alignment_overrides` blends the style's weights towards one
        "alignment_poles": {
            "lyric": {"acoustic_pause": 0.38, "asr_gap": 0.26, "sentence_end": 0.22, "beat_affinity": 0.02, "mdd_affinity": 0.06,
                      "breath": 0.10, "inside_word_penalty": 0.85, "singing_penalty": 0.50},
            "beat": {"acoustic_pause": 0.22, "asr_gap": 0.10, "sentence_end": 0.08, "beat_affinity": 0.32, "mdd_affinity": 0.12,
                     "breath": 0.10, "inside_word_penalty": 0.80, "singing_penalty": 0.50},
        },
    },
    "global_planner": {
        "enable": True, "hard_min_s": 2.0, "hard_max_s": 18.0, "target_min_s": 5.0, "target_max_s": 12.0,
        "vocal_risk_weight": 0.25, "beat_conflict_weight": 0.15, "max_candidates_per_second": 2.0, "rescue_enabled": True,
    },
    # mode `librosa_onset` (`expert.yaml:129-144`)
    "librosa_onset": {
        "use_vocal_separation": True,
        "silence": {"threshold_db": -40, "min_duration": 0.3},
        "density": "low",
        "density_custom": {"enable": False, "verse_bars": 4, "chorus_bars": 2},
        "energy_analysis": {"hop_length": 512, "chorus_percentile": 60, "chorus_peak_percentile": 80},
        "beat": {"time_signature": 4},
    },
    # mode `hybrid_mdd` (`expert.yaml:145-169`)
    "hybrid_mdd": {
        "beat_cut_density": "medium", "lib_alignment": "snap_to_beat", "snap_tolerance_ms": 200, "vad_protection": True,
        "chorus_force_snap": False,
        "density_presets": {
            "low": {"enable_beat_cuts": True, "energy_percentile": 90, "bars_per_cut": 4},
            "medium": {"enable_beat_cuts": True, "energy_percentile": 60, "bars_per_cut": 2},
            "high": {"enable_beat_cuts": True, "energy_percentile": 40, "bars_per_cut": 1},
        },
        "beat_detection": {"hop_length": 512, "time_signature": 4, "snap_to_pause_ms": 300},
        "labeling": {"lib_suffix": "_lib"},
    },
}

_runtime: Dict[str, Any] = {}
_explicit: Set[str] = set()       # the keys of `_runtime` that went in through `set_runtime_config(..., explicit=True)`
_MISSING = object()


def _lookup(tree: Dict[str, Any], path: str) -> Any:
    node: Any = tree
    for part in path.split("."):
        if isinstance(node, dict) and part in node:
            node = node[part]
        else:
            return _MISSING
    return node


def get_config(path: str, default: Any = None) -> Any:
    """The reference's `set_runtime_config` writes the override INTO the config tree (`config_manager.py:497-509`), so an
    override of a section (`{'segment_layout': {...}}`) replaces that subtree for every later child lookup, and an override
    of a child key set afterwards lands inside it.  `_runtime` keeps insertion order: the last write that covers `path`
    (the key itself, an ancestor, or descendants on top of either) wins."""
    parts = path.split(".")
    keys = list(_runtime)
    # the most recently written ancestor section (or the key itself) that is a dict-valued override, if any
    anc = [(keys.index(k), k) for k in (".".join(parts[:i]) for i in range(len(parts), 0, -1)) if k in _runtime]
    if anc:
        pos, key = max(anc)
        rest = path[len(key) + 1:] if len(path) > len(key) else ""
        node = _runtime[key]
        sub = _lookup(node, rest) if rest else node
        if rest and not isinstance(node, dict):
            sub = _MISSING
        value = copy.deepcopy(sub) if sub is not _MISSING else _MISSING
        prefix = path + "."
        later = {k[len(prefix):]: v for k, v in _runtime.items() if k.startswith(prefix) and keys.index(k) > pos}
        exact_later = path in _runtime and keys.index(path) > pos
        if exact_later:
            value = copy.deepcopy(_runtime[path])
        if later:
            value = {} if value is _MISSING or not isinstance(value, dict) else value
            for subkey, v in later.items():
                tgt = value
                sp = subkey.split(".")
                for p_ in sp[:-1]:
                    tgt = tgt.setdefault(p_, {})
                tgt[sp[-1]] = copy.deepcopy(v)
        return default if value is _MISSING else value
    # an override of a child key only
    base = _lookup(DEFAULTS, path)
    prefix = path + "."
    children = {k[len(prefix):]: v for k, v in _runtime.items() if k.startswith(prefix)}
    if base is _MISSING and not children:
        return default
    value = copy.deepcopy(base) if base is not _MISSING else {}
    for sub, v in children.items():
        node = value
        parts = sub.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = copy.deepcopy(v)
    return value


def _env_override(value: Any, env_key: str, convert) -> Any:
    """`_get_with_env_override` (`config_manager.py:582-602`): the environment wins; a value that does not convert is ignored."""
    raw = os.environ.get(env_key)
    if raw is None:
        return value
    try:
        return convert(raw)
    except (ValueError, TypeError):
        return value


def get_librosa_onset_config() -> Dict[str, Any]:
    """`get_librosa_onset_config` (`config_manager.py:527-579`): the `librosa_onset` section with the reference's literal
    defaults for absent keys, and the `AUDIOCUT_*` environment overrides on top of four of them."""
    base = get_config("librosa_onset", {}) or {}
    silence = base.get("silence", {})
    return {
        "use_vocal_separation": _env_override(base.get("use_vocal_separation", True), "AUDIOCUT_LIBROSA_USE_VOCAL",
                                              lambda x: x.lower() == "true"),
        "silence": {
            "threshold_db": _env_override(silence.get("threshold_db", -40), "AUDIOCUT_SILENCE_THRESHOLD_DB", float),
            "min_duration": _env_override(silence.get("min_duration", 0.3), "AUDIOCUT_SILENCE_MIN_DURATION", float),
        },
        "density": _env_override(base.get("density", "medium"), "AUDIOCUT_DENSITY", str),
        "density_custom": base.get("density_custom", {"enable": False, "verse_bars": 4, "chorus_bars": 2}),
        "energy_analysis": base.get("energy_analysis", {"hop_length": 512, "chorus_percentile": 60, "chorus_peak_percentile": 80}),
        "beat": base.get("beat", {"time_signature": 4}),
    }


def get_hybrid_mdd_config(density_override: Any = None) -> Dict[str, Any]:
    """`get_hybrid_mdd_config` (`config_manager.py:605-669`): `density_override` > environment > the `hybrid_mdd` section > the
    reference's literal defaults.  A density without a preset takes the `medium` preset (and keeps its own name)."""
    base = get_config("hybrid_mdd", {}) or {}
    density = density_override or _env_override(base.get("beat_cut_density", "medium"), "AUDIOCUT_HYBRID_DENSITY", str)
    presets = base.get("density_presets", {})
    preset = presets.get(density, presets.get("medium", {}))
    truthy = lambda x: str(x).lower() in ("true", "1", "yes")
    beat = base.get("beat_detection", {})
    return {
        "density": density,
        "enable_beat_cuts": preset.get("enable_beat_cuts", True),
        "energy_percentile": preset.get("energy_percentile", 70),
        "bars_per_cut": preset.get("bars_per_cut", 2),
        "lib_alignment": _env_override(base.get("lib_alignment", "snap_to_beat"), "AUDIOCUT_HYBRID_LIB_ALIGNMENT", str),
        "snap_tolerance_ms": _env_override(base.get("snap_tolerance_ms", 300), "AUDIOCUT_SNAP_TOLERANCE_MS", int),
        "vad_protection": _env_override(base.get("vad_protection", True), "AUDIOCUT_VAD_PROTECTION", truthy),
        "chorus_force_snap": _env_override(base.get("chorus_force_snap", False), "AUDIOCUT_CHORUS_FORCE_SNAP", truthy),
        "beat_detection": {"hop_length": beat.get("hop_length", 512), "time_signature": beat.get("time_signature", 4),
                           "snap_to_pause_ms": beat.get("snap_to_pause_ms", 300)},
        "labeling": {"lib_suffix": base.get("labeling", {}).get("lib_suffix", "_lib")},
    }


def set_runtime_config(overrides: Dict[str, Any], *, explicit: bool = True) -> None:
    """Dotted-key overrides (reference: config_manager.py:497-509).  A key written again moves to the end (last write wins).
    `explicit` (the default, and what the reference's function does): the keys are reported by `get_runtime_override_keys`.
    `explicit=False` is the reference API's own way in - it writes device, layout, intent and `runtime_overrides` straight into
    the tree (`api.py:147-175`), so they override without counting as stated by the caller; a key the caller had marked before
    stays marked, as it does there."""
    for k, v in (overrides or {}).items():
        _runtime.pop(str(k), None)
        _runtime[str(k)] = v
        if explicit:
            _explicit.add(str(k))


def get_runtime_override_keys() -> Set[str]:
    """The dotted keys set through `set_runtime_config` and still in force (`config_manager.py:512-515`), as a copy."""
    return set(_explicit)


def reset_runtime_config() -> None:
    _runtime.clear()
    _explicit.clear()


class _Snapshot(dict):
    """`snapshot()`'s value: the override map, as before, and with it the explicit-key set of that moment."""
    explicit: frozenset = frozenset()


def snapshot() -> Dict[str, Any]:
    saved = _Snapshot(_runtime)
    saved.explicit = frozenset(_explicit)
    return saved


def restore(saved: Dict[str, Any]) -> None:
    """Back to `saved`: the overrides, and the explicit keys `snapshot()` recorded with them (a plain dict: those of its keys that
    were explicit until now)."""
    marks = getattr(saved, "explicit", None)
    keep = set(marks) if marks is not None else {k for k in _explicit if k in saved}
    _runtime.clear()
    _runtime.update(saved)
    _explicit.clear()
    _explicit.update(k for k in keep if k in _runtime)
