"""The two cut strategies of mode `hybrid_mdd` — mirrors `src/vocal_smart_splitter/core/strategies/{base,snap_to_beat_strategy,
beat_only_strategy}.py` of the reference (`SegmentationContext`, `SegmentationResult`, `deduplicate_and_convert_cuts`,
`SnapToBeatStrategy`, `BeatOnlyStrategy`; names, fields, defaults and quirks kept).

One difference in what they are given: the reference asks `is_quiet_vocal_window` about one beat at a time, and every question
re-reads the whole vocal stem.  Here the orchestrator gates every beat and bar line of the track in ONE `ac_quiet_gate_meansq`
launch before a strategy runs, and the strategies look the answers up: `SegmentationContext.quiet_gate` maps a window's centre
sample `int(round(t * sr))` to the reference's decision for that time.  A time that was not gated is a `KeyError`, never a guess.

Quirks kept on purpose: the snap tolerance is clamped to 0.4 x the mean beat interval; `_find_bar_index` answers the last bar for
a time outside every bar; a blocked chorus cut in `beat_only` leaves `bars_since_last_cut` running; `cut_is_lib[i]` is looked up by
the position in the unfiltered cut list after the `seen` filter; `deduplicate_and_convert_cuts` re-aligns its flags by the 0.1 s
rule when cuts collapse onto one sample.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from ..analysis.chorus_regions import detect_chorus_regions

logger = logging.getLogger(__name__)


@dataclass
class SegmentationContext:
    """What a strategy reads.  `audio` only lends its length; `quiet_gate` stands where the reference's `vocal_track` stands."""
    audio: np.ndarray
    sample_rate: int
    tempo: float
    beat_times: np.ndarray
    bar_times: np.ndarray
    bar_duration: float
    mdd_cut_points_samples: List[int]
    energy_threshold: float
    bar_energies: List[float]
    bar_spectral_centroids: List[float] = field(default_factory=list)
    bar_spectral_bandwidths: List[float] = field(default_factory=list)
    quiet_gate: Mapping[int, bool] = field(default_factory=dict)
    config: Dict[str, Any] = field(default_factory=dict)


@dataclass
class SegmentationResult:
    cut_points_samples: List[int]
    lib_flags: List[bool]
    metadata: Optional[Dict[str, Any]] = None


def gate_center(time: float, sample_rate: int) -> int:
    """The centre sample of the window `is_quiet_vocal_window` reads around `time` (`base.py:173`)."""
    return int(round(time * sample_rate))


def gate_half_window(sample_rate: int, guard_win_ms: float) -> int:
    """`base.py:174`."""
    return max(1, int(round(sample_rate * guard_win_ms / 1000.0)))


def gate_decisions(block_ms: np.ndarray, point_ms: np.ndarray, point_count: np.ndarray, guard_db: float):
    """`is_quiet_vocal_window`'s arithmetic on the kernel's mean squares -> (floor_db, point_db per centre, quiet per centre).
    `_vocal_floor_db` (`base.py:185-195`): the 5th percentile of sqrt(mean square) + 1e-12 over the blocks, -120 dB without
    blocks; `_rms_db` (`:198-200`); a window without samples is quiet (`:177-178`), and so is every window of an empty track."""
    block_ms = np.asarray(block_ms, dtype=np.float64)
    if block_ms.size:
        floor_db = float(20.0 * np.log10(np.percentile(np.sqrt(block_ms) + 1e-12, 5)))
    else:
        floor_db = -120.0
    point_db = 20.0 * np.log10(np.sqrt(np.asarray(point_ms, dtype=np.float64)) + 1e-12)
    quiet = (np.asarray(point_count) == 0) | (point_db <= floor_db + float(guard_db))
    return floor_db, point_db, quiet


def _is_quiet(gate: Mapping[int, bool], sample_rate: int, time: float) -> bool:
    if sample_rate <= 0:
        return True
    return bool(gate[gate_center(time, sample_rate)])


def deduplicate_and_convert_cuts(cut_with_flags: List[Tuple[float, bool]], sample_rate: int, audio_len: int, *,
                                 time_tolerance_s: float = 0.1) -> Tuple[List[int], List[bool]]:
    """`base.py:100-158`: unique times in order -> samples (truncated) -> one flag per segment, the flag of the cut that ends it."""
    if sample_rate <= 0 or audio_len < 0:
        return [0, max(0, audio_len)], []
    audio_duration = audio_len / float(sample_rate)
    if not cut_with_flags:
        cut_with_flags = [(0.0, False), (audio_duration, False)]
    unique: List[Tuple[float, bool]] = []
    seen = set()
    for t, flag in cut_with_flags:
        if t in seen:
            continue
        seen.add(t)
        unique.append((float(t), bool(flag)))
    unique.sort(key=lambda x: x[0])
    if not unique or unique[0][0] != 0.0:
        unique.insert(0, (0.0, False))
    if unique[-1][0] != audio_duration:
        unique.append((audio_duration, False))
    cut_points_samples: List[int] = []
    lib_flags: List[bool] = []
    for i, (t, is_lib) in enumerate(unique):
        sample_idx = int(t * sample_rate)
        sample_idx = max(0, min(sample_idx, audio_len))
        cut_points_samples.append(sample_idx)
        if i > 0:
            lib_flags.append(is_lib)
    if cut_points_samples[0] != 0:
        cut_points_samples.insert(0, 0)
        lib_flags.insert(0, False)
    if cut_points_samples[-1] != audio_len:
        cut_points_samples.append(audio_len)
    cut_points_samples = sorted(set(cut_points_samples))
    num_segments = len(cut_points_samples) - 1
    if len(lib_flags) != num_segments:          # cuts collapsed onto one sample: flag a segment whose end is within 0.1 s of a lib cut
        time_to_lib = {t: is_lib for t, is_lib in unique}
        lib_flags = []
        for i in range(num_segments):
            end_time = cut_points_samples[i + 1] / float(sample_rate)
            lib_flags.append(any(abs(end_time - t) < time_tolerance_s and flag for t, flag in time_to_lib.items()))
    return cut_points_samples, lib_flags


def _chorus_bars(context: SegmentationContext, energy_percentile: float):
    bar_energies = context.bar_energies
    if bar_energies:
        energy_threshold = float(np.percentile(bar_energies, energy_percentile))
    else:
        energy_threshold = context.energy_threshold
    return detect_chorus_regions(bar_energies, energy_threshold, bar_centroids=context.bar_spectral_centroids,
                                 bar_bandwidths=context.bar_spectral_bandwidths)


def _flagged(cuts: Sequence[float], cut_is_lib: Sequence[bool], audio_duration: float) -> List[Tuple[float, bool]]:
    """Both strategies' closing step: the interior cuts without repeats, each with the flag found at ITS index in the list
    before the filter."""
    out: List[Tuple[float, bool]] = [(0.0, False)]
    seen = {0.0}
    for i, t in enumerate(cuts[1:-1]):
        if t in seen:
            continue
        seen.add(t)
        out.append((t, cut_is_lib[i] if i < len(cut_is_lib) else False))
    out.append((audio_duration, False))
    return out


class SnapToBeatStrategy:
    """Plan C (`snap_to_beat_strategy.py:24-324`): inside chorus bars an MDD cut moves to the nearest beat within the tolerance
    whose vocal window is quiet, and the segment it ends is `_lib`; everywhere else the MDD cut stays."""

    @property
    def name(self) -> str:
        return "snap_to_beat"

    def generate_cut_points(self, context: SegmentationContext) -> SegmentationResult:
        config = context.config
        snap_tolerance_ms = float(config.get("snap_tolerance_ms", 300))
        snap_tolerance_s = snap_tolerance_ms / 1000.0
        vad_protection = bool(config.get("vad_protection", True))
        chorus_force_snap = bool(config.get("chorus_force_snap", False))
        min_segment_s = float(config.get("min_segment_s", 2.0))
        energy_percentile = float(config.get("energy_percentile", 70))
        sample_rate = context.sample_rate
        audio_len = len(context.audio)
        audio_duration = audio_len / float(sample_rate)
        beat_times = context.beat_times
        bar_times = context.bar_times
        gate = context.quiet_gate
        mdd_cut_times = [s / float(sample_rate) for s in context.mdd_cut_points_samples]
        high_energy_bars = _chorus_bars(context, energy_percentile)

        if len(beat_times) >= 2:
            avg_beat_interval = float(np.mean(np.diff(beat_times)))
        else:
            avg_beat_interval = context.bar_duration / 4 if context.bar_duration else 0.5
        if avg_beat_interval > 0:
            max_snap_tolerance_s = 0.4 * avg_beat_interval
            if snap_tolerance_s > max_snap_tolerance_s:
                snap_tolerance_s = max_snap_tolerance_s
                snap_tolerance_ms = snap_tolerance_s * 1000.0

        snapped_cuts: List[float] = [0.0]
        cut_is_lib: List[bool] = []
        snap_stats = {"snapped": 0, "vad_blocked": 0, "too_far": 0, "low_energy": 0}
        for mdd_time in mdd_cut_times:
            if mdd_time <= 0 or mdd_time >= audio_duration:
                continue
            is_high_energy = self._find_bar_index(mdd_time, bar_times) in high_energy_bars
            nearest_beat_time = self._find_nearest_beat(mdd_time, beat_times)
            distance_to_beat = abs(mdd_time - nearest_beat_time)
            should_snap = False
            final_cut_time = mdd_time
            if not is_high_energy:
                snap_stats["low_energy"] += 1
            elif distance_to_beat <= snap_tolerance_s:
                quiet_beat_time: Optional[float] = nearest_beat_time
                if vad_protection and not chorus_force_snap:
                    quiet_beat_time = self._find_quiet_beat_within_tolerance(mdd_time, beat_times, gate, sample_rate, snap_tolerance_s)
                if quiet_beat_time is None:
                    snap_stats["vad_blocked"] += 1
                else:
                    should_snap = True
                    final_cut_time = quiet_beat_time
                    snap_stats["snapped"] += 1
            else:
                snap_stats["too_far"] += 1
            if snapped_cuts and final_cut_time - snapped_cuts[-1] < min_segment_s:
                continue
            snapped_cuts.append(final_cut_time)
            cut_is_lib.append(should_snap)

        if config.get("density", "medium") == "high" and high_energy_bars:      # bar-length `_lib` segments in the chorus
            for bar_idx in high_energy_bars:
                bar_start = bar_times[bar_idx]
                bar_end = bar_times[bar_idx + 1] if bar_idx + 1 < len(bar_times) else audio_duration
                beats_in_bar = [b for b in beat_times if bar_start <= b < bar_end]
                if beats_in_bar:
                    beat_cut = float(beats_in_bar[0])
                    min_distance = min(abs(beat_cut - c) for c in snapped_cuts) if snapped_cuts else float("inf")
                    if min_distance > min_segment_s * 0.5:
                        if vad_protection and not chorus_force_snap and not _is_quiet(gate, sample_rate, beat_cut):
                            snap_stats["vad_blocked"] += 1
                            continue
                        snapped_cuts.append(beat_cut)
                        cut_is_lib.append(True)
        snapped_cuts.append(audio_duration)
        logger.info("[SNAP_TO_BEAT] %d snapped, %d VAD-blocked, %d low-energy, %d too far", snap_stats["snapped"],
                    snap_stats["vad_blocked"], snap_stats["low_energy"], snap_stats["too_far"])

        cut_points_samples, lib_flags = deduplicate_and_convert_cuts(_flagged(snapped_cuts, cut_is_lib, audio_duration),
                                                                     sample_rate, audio_len)
        num_segments = len(cut_points_samples) - 1
        segment_durations = [(cut_points_samples[i + 1] - cut_points_samples[i]) / float(sample_rate) for i in range(num_segments)]
        lib_count = sum(1 for f in lib_flags if f)
        return SegmentationResult(cut_points_samples=cut_points_samples, lib_flags=lib_flags, metadata={
            "strategy": self.name, "snap_tolerance_ms": snap_tolerance_ms, "vad_protection": vad_protection,
            "chorus_force_snap": chorus_force_snap, "snapped_count": lib_count, "kept_mdd_count": num_segments - lib_count,
            "snap_stats": snap_stats, "segment_durations": segment_durations})

    def _find_nearest_beat(self, time: float, beat_times: np.ndarray) -> float:
        if len(beat_times) == 0:
            return time
        return float(beat_times[np.abs(beat_times - time).argmin()])

    def _find_bar_index(self, time: float, bar_times: np.ndarray) -> int:
        for i in range(len(bar_times) - 1):
            if bar_times[i] <= time < bar_times[i + 1]:
                return i
        return len(bar_times) - 2 if len(bar_times) > 1 else 0

    def _find_quiet_beat_within_tolerance(self, time: float, beat_times: np.ndarray, gate: Mapping[int, bool], sample_rate: int,
                                          tolerance_s: float) -> Optional[float]:
        """The beat nearest to `time` among those within the tolerance whose window is quiet, or None."""
        if len(beat_times) == 0:
            return None
        candidates = [float(beat) for beat in beat_times if abs(float(beat) - time) <= tolerance_s]
        candidates.sort(key=lambda beat: abs(beat - time))
        for beat in candidates:
            if _is_quiet(gate, sample_rate, beat):
                return beat
        return None


class BeatOnlyStrategy:
    """Plan B (`beat_only_strategy.py:24-201`): chorus bars are cut at bar ends every `bars_per_cut` bars (`_lib`), verse bars at
    the first MDD cut inside them, or at a bar end after twice as many bars without one."""

    @property
    def name(self) -> str:
        return "beat_only"

    def generate_cut_points(self, context: SegmentationContext) -> SegmentationResult:
        config = context.config
        bars_per_cut = int(config.get("bars_per_cut", 2))
        min_segment_s = float(config.get("min_segment_s", 2.0))
        energy_percentile = float(config.get("energy_percentile", 70))
        vad_protection = bool(config.get("vad_protection", True))
        chorus_force_snap = bool(config.get("chorus_force_snap", False))
        sample_rate = context.sample_rate
        audio_len = len(context.audio)
        audio_duration = audio_len / float(sample_rate)
        bar_times = context.bar_times
        gate = context.quiet_gate
        high_energy_bars = _chorus_bars(context, energy_percentile)

        cut_times: List[float] = [0.0]
        cut_is_lib: List[bool] = []
        vad_blocked = 0
        mdd_cut_times = [s / float(sample_rate) for s in context.mdd_cut_points_samples]
        bars_since_last_cut = 0
        last_cut_time = 0.0
        for bar_idx in range(len(bar_times) - 1):
            bar_start = bar_times[bar_idx]
            bar_end = bar_times[bar_idx + 1] if bar_idx + 1 < len(bar_times) else audio_duration
            bars_since_last_cut += 1
            if bar_idx in high_energy_bars:
                if bars_since_last_cut >= bars_per_cut:
                    cut_time = float(bar_end)
                    if cut_time <= audio_duration and cut_time - last_cut_time >= min_segment_s:
                        if vad_protection and not chorus_force_snap and not _is_quiet(gate, sample_rate, cut_time):
                            vad_blocked += 1
                            continue                    # the counter keeps running: the next bar end is tried at once
                        cut_times.append(cut_time)
                        cut_is_lib.append(True)
                        last_cut_time = cut_time
                        bars_since_last_cut = 0
            else:
                for mdd_t in mdd_cut_times:
                    if bar_start <= mdd_t < bar_end and mdd_t > last_cut_time + min_segment_s:
                        cut_times.append(mdd_t)
                        cut_is_lib.append(False)
                        last_cut_time = mdd_t
                        bars_since_last_cut = 0
                        break
                else:
                    if bars_since_last_cut >= bars_per_cut * 2:
                        cut_time = float(bar_end)
                        if cut_time <= audio_duration and cut_time - last_cut_time >= min_segment_s:
                            cut_times.append(cut_time)
                            cut_is_lib.append(False)
                            last_cut_time = cut_time
                            bars_since_last_cut = 0
        cut_times.append(audio_duration)

        cut_points_samples, lib_flags = deduplicate_and_convert_cuts(_flagged(cut_times, cut_is_lib, audio_duration),
                                                                     sample_rate, audio_len)
        num_segments = len(cut_points_samples) - 1
        segment_durations = [(cut_points_samples[i + 1] - cut_points_samples[i]) / float(sample_rate) for i in range(num_segments)]
        lib_count = sum(1 for f in lib_flags if f)
        return SegmentationResult(cut_points_samples=cut_points_samples, lib_flags=lib_flags, metadata={
            "strategy": self.name, "bars_per_cut": bars_per_cut, "num_bars": len(bar_times), "high_energy_bars": len(high_energy_bars),
            "lib_segment_count": lib_count, "vad_blocked": vad_blocked, "segment_durations": segment_durations})


__all__ = ["SegmentationContext", "SegmentationResult", "SnapToBeatStrategy", "BeatOnlyStrategy", "deduplicate_and_convert_cuts",
           "gate_center", "gate_half_window", "gate_decisions"]
