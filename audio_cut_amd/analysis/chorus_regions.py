"""Chorus bars: runs of consecutive "high" bars, where high is either a plain energy threshold or a fused score of the
per-bar energy, spectral centroid and spectral bandwidth — mirrors `src/audio_cut/analysis/chorus_regions.py:16-99` of the
reference (names and signatures kept; VPBD's beat candidates use the energy branch, the hybrid strategies the fused one).

Pure host logic over a few hundred bars; the per-bar lists come from `analysis.beat_analyzer` (`ac_bar_means3`).
"""
from __future__ import annotations

from typing import Iterable, Optional, Set, Tuple

import numpy as np

FUSION_PERCENTILE = 60
# (energy, centroid, bandwidth) weights by the coefficient of variation of the bar energies: a track whose loudness hardly
# moves is told apart by its spectrum, a track with wide dynamics by its energy
WEIGHTS_LOW_DYNAMICS = (0.3, 0.4, 0.3)       # cv < 0.15
WEIGHTS_HIGH_DYNAMICS = (0.6, 0.2, 0.2)      # cv > 0.4
WEIGHTS_BALANCED = (0.5, 0.25, 0.25)


def _normalize(values: Iterable[float]) -> np.ndarray:
    """Min-max to [0, 1] as float32; a range of 1e-6 or less gives zeros."""
    arr = np.asarray(list(values), dtype=np.float32)
    if arr.size == 0:
        return arr
    lo, hi = float(np.min(arr)), float(np.max(arr))
    if hi - lo > 1e-6:
        return (arr - lo) / (hi - lo)
    return np.zeros_like(arr)


def energy_cv(energies: np.ndarray) -> float:
    return float(np.std(energies) / (np.mean(energies) + 1e-6))


def fusion_weights(cv: float) -> Tuple[float, float, float]:
    if cv < 0.15:
        return WEIGHTS_LOW_DYNAMICS
    if cv > 0.4:
        return WEIGHTS_HIGH_DYNAMICS
    return WEIGHTS_BALANCED


def fused_scores(bar_energies: Iterable[float], bar_centroids: Iterable[float], bar_bandwidths: Iterable[float]):
    """-> (score per bar float32, its 60th percentile, cv of the energies): what the fusion branch decides on."""
    energies = np.asarray(list(bar_energies), dtype=np.float32)
    cv = energy_cv(energies)
    w_e, w_c, w_b = fusion_weights(cv)
    score = _normalize(energies) * w_e + _normalize(bar_centroids) * w_c + _normalize(bar_bandwidths) * w_b
    return score, float(np.percentile(score, FUSION_PERCENTILE)), cv


def _continuous_regions(is_high: Iterable[bool], *, min_consecutive_bars: int) -> Set[int]:
    """Indices inside runs of at least `min_consecutive_bars` true flags."""
    flags = [bool(f) for f in is_high]
    bars: Set[int] = set()
    run_start = None
    for i, flag in enumerate(flags + [False]):           # the sentinel closes a run that reaches the last bar
        if flag:
            if run_start is None:
                run_start = i
        elif run_start is not None:
            if i - run_start >= min_consecutive_bars:
                bars.update(range(run_start, i))
            run_start = None
    return bars


def detect_chorus_regions(bar_energies: Iterable[float], energy_threshold: float, *, min_consecutive_bars: int = 4,
                          bar_centroids: Optional[Iterable[float]] = None,
                          bar_bandwidths: Optional[Iterable[float]] = None) -> Set[int]:
    """Bars that belong to runs of >= `min_consecutive_bars` high bars.  With centroid and bandwidth lists as long as the
    energies, high = fused score >= its 60th percentile (`energy_threshold` is not used); otherwise high = energy >= threshold."""
    energies = np.asarray(list(bar_energies), dtype=np.float32)
    if energies.size == 0:
        return set()
    centroids = list(bar_centroids) if bar_centroids is not None else []
    bandwidths = list(bar_bandwidths) if bar_bandwidths is not None else []
    if centroids and bandwidths and len(centroids) == len(energies):
        score, threshold, _ = fused_scores(energies, centroids, bandwidths)
        is_high = score >= threshold
    else:
        is_high = energies >= float(energy_threshold)
    return _continuous_regions(is_high, min_consecutive_bars=max(1, int(min_consecutive_bars)))


__all__ = ["detect_chorus_regions", "fused_scores", "fusion_weights", "energy_cv"]
