"""Host rules of the `librosa_onset` mode ("smart music segmentation v2"): the scalar part of the reference's
`_process_librosa_onset_split` (`src/vocal_smart_splitter/core/seamless_splitter.py:1097-1250`) as pure, GPU-free functions.

The series these rules read (per-bar mean RMS, per-frame silent flags) come from `ac_bar_energy_silence`; what is here runs
over a few hundred bars and ~20 k flags per track.  The reference's quirks are kept, not fixed: a silence still open at the
end of the track is dropped, the cut inside a silence is the midpoint of FRAME times, `int(t * sr)` truncates, and the
short-segment merge always keeps the last point.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np

DENSITY_PRESETS = {
    "low": {"verse_bars": 8, "chorus_bars": 4},
    "medium": {"verse_bars": 4, "chorus_bars": 2},
    "high": {"verse_bars": 2, "chorus_bars": 1},
}


def bar_grid(duration: float, bar_duration: float) -> np.ndarray:
    """`bar_times_all` (`:1105`): bar starts from 0 to the first one at or past the end of the track."""
    return np.arange(0, duration + bar_duration, bar_duration)


def rms_frame_times(n_frames: int, sr: int, hop_length: int) -> np.ndarray:
    """`librosa.frames_to_time(np.arange(n_frames), sr, hop_length)` (`:1102`), float64."""
    return (np.arange(n_frames) * hop_length).astype(int) / float(sr)


def bar_frame_ranges(rms_times: np.ndarray, bar_times: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Half-open frame ranges [lo_b, hi_b) of the mask `(rms_times >= bar_times[b]) & (rms_times < bar_times[b + 1])`
    (`:1113`): `rms_times` is sorted, so the first frame at or past each bar time bounds the same sets."""
    edges = np.searchsorted(np.asarray(rms_times, dtype=np.float64), np.asarray(bar_times, dtype=np.float64), side="left")
    return edges[:-1].astype(np.int64), edges[1:].astype(np.int64)


def classify_bars(bar_energies: Sequence[float], chorus_percentile: float = 60, chorus_peak_percentile: float = 80):
    """`:1119-1138` -> (bar types, chorus threshold, peak threshold); the thresholds are percentiles of these very energies."""
    energies = [float(e) for e in bar_energies]
    if energies:
        thr_chorus = float(np.percentile(energies, chorus_percentile))
        thr_peak = float(np.percentile(energies, chorus_peak_percentile))
    else:
        thr_chorus = thr_peak = 0.0
    types: List[str] = []
    for energy in energies:
        if energy >= thr_peak:
            types.append("chorus_peak")
        elif energy >= thr_chorus:
            types.append("chorus")
        else:
            types.append("verse")
    return types, thr_chorus, thr_peak


def silence_boundaries(flags: Sequence[bool], rms_times: np.ndarray, duration: float, min_duration: float) -> List[float]:
    """`:1151-1164`: the midpoint of every silent run of at least `min_duration` seconds that ENDS inside the track."""
    out: List[float] = []
    in_silence = False
    start = 0.0
    n_times = len(rms_times)
    for i, silent in enumerate(flags):
        t = float(rms_times[i]) if i < n_times else duration
        if silent and not in_silence:
            in_silence = True
            start = t
        elif not silent and in_silence:
            in_silence = False
            length = t - start
            if length >= min_duration:
                out.append(start + length / 2)
    return out


def density_config(lo_config: Mapping) -> Dict[str, int]:
    """`:1168-1186`: `density_custom` when enabled, else the preset (an unknown name means medium)."""
    custom = lo_config.get("density_custom", {}) or {}
    if custom.get("enable", False):
        return {"verse_bars": custom.get("verse_bars", 4), "chorus_bars": custom.get("chorus_bars", 2)}
    return dict(DENSITY_PRESETS.get(lo_config.get("density"), DENSITY_PRESETS["medium"]))


def plan_bar_cuts(bar_times: Sequence[float], bar_types: Sequence[str], silence_boundaries: Sequence[float],
                  density_cfg: Mapping[str, int], duration: float, min_segment_s: float) -> List[float]:
    """`:1190-1238`: a cut every `chorus_bars` / `verse_bars` bars, forced at the first bar line behind a silence; then every
    silence midpoint itself, `sorted(set())`, and the merge of segments shorter than `min_segment_s`."""
    cut_times: List[float] = [0.0]
    last_cut = 0.0
    since = 0
    for idx, bar_time in enumerate(bar_times[1:]):
        since += 1
        bar_type = bar_types[idx] if idx < len(bar_types) else "verse"
        need = density_cfg["chorus_bars"] if "chorus" in bar_type else density_cfg["verse_bars"]
        cut = since >= need
        for s in silence_boundaries:
            if last_cut < s <= bar_time:
                cut = True
                break
        if cut:
            cut_times.append(float(bar_time))
            last_cut = bar_time
            since = 0
    for s in silence_boundaries:
        if s not in cut_times and 0 < s < duration:
            cut_times.append(s)
    cut_times.append(duration)
    cut_times = sorted(set(cut_times))
    merged: List[float] = [cut_times[0]]
    for t in cut_times[1:]:
        if t - merged[-1] >= min_segment_s:
            merged.append(t)
        elif t == cut_times[-1]:
            merged[-1] = t
    return merged


def to_sample_points(cut_times: Sequence[float], sr: int, n: int) -> List[int]:
    """`:1243-1250`: interior times as `int(t * sr)` (truncated), kept when strictly inside the track."""
    points = [0]
    for t in cut_times[1:-1]:
        idx = int(t * sr)
        if 0 < idx < n:
            points.append(idx)
    points.append(int(n))
    return sorted(set(points))


def label_segments(vocal_sumsq: Sequence[float], inst_sumsq, cut_points: Sequence[int]) -> List[bool]:
    """`:1253-1273` from per-segment sums of squares: human when `vocal_rms > 0.3 * inst_rms`; with no instrumental stem
    (`inst_sumsq` None) when `vocal_rms > 0.01`; with no vocal stem (`vocal_sumsq` None) every segment is human."""
    n_seg = len(cut_points) - 1
    if vocal_sumsq is None:
        return [True] * n_seg
    flags: List[bool] = []
    for i in range(n_seg):
        size = int(cut_points[i + 1]) - int(cut_points[i])
        vocal_rms = float(np.sqrt(float(vocal_sumsq[i]) / size))
        if inst_sumsq is not None:
            flags.append(bool(vocal_rms > float(np.sqrt(float(inst_sumsq[i]) / size)) * 0.3))
        else:
            flags.append(bool(vocal_rms > 0.01))
    return flags


__all__ = ["DENSITY_PRESETS", "bar_grid", "rms_frame_times", "bar_frame_ranges", "classify_bars", "silence_boundaries",
           "density_config", "plan_bar_cuts", "to_sample_points", "label_segments"]
