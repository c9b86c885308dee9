"""Beat / bar analysis of a mix: tempo, bar boundaries and, per bar, the mean RMS energy, spectral centroid and spectral
bandwidth, plus the bars at or above an energy percentile — mirrors `src/audio_cut/analysis/beat_analyzer.py:21-334` of the
reference (`BeatAnalysisResult`, `analyze_beats`, `BeatAnalyzer`; names, fields and defaults kept).

Where the work runs: the three framewise series are two passes over the mix resident in HBM (`ac_frame_rms` at 2048 / hop and
`ac_stft2048_centroid_bandwidth`), queued as soon as the mix is on the device and before the host has decided anything; the
host then turns the bar boundaries into frame ranges and one `ac_bar_means3` launch returns the 3 x n_bars means in one
download.  Without cached beats the tempo and the beats come from the mix's median onset envelope and the device beat
tracker, as in the `librosa_onset` mode.  There is no host fallback: no GPU or no library raises `_native.NativeError`.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from typing import List, Optional, Set, Tuple, TYPE_CHECKING

import numpy as np

from .. import _native

if TYPE_CHECKING:
    from .features_cache import TrackFeatureCache

logger = logging.getLogger(__name__)

RMS_FRAME = 2048           # librosa.feature.rms's default frame, the STFT's n_fft: both series have 1 + n // hop frames
DEFAULT_BPM = 120.0


@dataclass
class BeatAnalysisResult:
    tempo: float                                    # BPM
    beat_times: np.ndarray                          # seconds
    bar_times: np.ndarray                           # bar boundaries in seconds (n_bars + 1 of them)
    bar_duration: float                             # seconds per bar at `tempo`
    bar_energies: List[float]                       # mean RMS per bar
    bar_spectral_centroids: List[float] = field(default_factory=list)      # mean centroid per bar, Hz
    bar_spectral_bandwidths: List[float] = field(default_factory=list)     # mean bandwidth per bar, Hz
    high_energy_bars: Set[int] = field(default_factory=set)                # bars with energy >= energy_threshold
    energy_threshold: float = 0.0
    num_beats: int = field(default=0)
    num_bars: int = field(default=0)

    def __post_init__(self):
        self.num_beats = len(self.beat_times) if self.beat_times is not None else 0
        self.num_bars = len(self.bar_times) - 1 if self.bar_times is not None and len(self.bar_times) > 1 else 0


def _ensure_mono(audio: np.ndarray) -> np.ndarray:
    if audio.ndim == 1:
        return audio
    if audio.ndim == 2:
        return np.mean(audio, axis=0)
    return audio.reshape(-1)


def _generate_bar_boundaries(beat_times: np.ndarray, audio_duration: float, time_signature: int = 4) -> np.ndarray:
    """Every `time_signature`-th beat starts a bar and the end of the track closes the last one.  With fewer beats than one
    bar holds there is nothing to group: a regular grid from 0 at the beats' mean spacing (120 BPM without two beats)."""
    if len(beat_times) < time_signature:
        if len(beat_times) >= 2:
            bar_duration = float(np.mean(np.diff(beat_times))) * time_signature
        else:
            bar_duration = 60.0 / DEFAULT_BPM * time_signature
        return np.arange(0, audio_duration + bar_duration, bar_duration)
    starts = [float(t) for t in beat_times[::time_signature]]
    return np.array(starts + [float(audio_duration)])


def frame_times(n_frames: int, sr: int, hop_length: int) -> np.ndarray:
    """`librosa.frames_to_time(np.arange(n_frames), sr=sr, hop_length=hop_length)`, float64."""
    return (np.arange(n_frames) * hop_length).astype(int) / float(sr)


def bar_frame_ranges(times: np.ndarray, bar_times: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Half-open frame ranges [lo_i, hi_i) holding the frames of the mask `(times >= bar_times[i]) & (times < bar_times[i + 1])`.
    `times` is sorted, so the first frame at or past a boundary splits it the way the comparison does, boundary by boundary;
    a bar whose end is not after its start comes out with hi <= lo - empty, like its mask."""
    edges = np.searchsorted(np.asarray(times, dtype=np.float64), np.asarray(bar_times, dtype=np.float64), side="left")
    return edges[:-1].astype(np.int64), edges[1:].astype(np.int64)


def _mono_on_device(ctx: "_native.Context", audio: np.ndarray, audio_dev):
    """The mono mix as a 1-D float32 device tensor: `audio_dev` when it is one, the channel mean of a [2, N] one, else an upload."""
    if audio_dev is not None:
        if audio_dev.dim() == 1:
            return audio_dev
        if audio_dev.dim() == 2 and audio_dev.shape[0] == 2:
            import torch
            return torch.add(audio_dev[0], audio_dev[1]).mul_(0.5)          # float32 (L + R) / 2: np.mean over two rows
        raise _native.NativeError("audio_dev must be a mono [n] or a planar [2, n] tensor")
    return ctx.to_device(np.ascontiguousarray(audio, dtype=np.float32))


def queue_frame_series(ctx: "_native.Context", mix_dev, sr: int, hop_length: int):
    """Launch the two passes over the mix on the current stream -> (rms float32, centroid float64, bandwidth float64), device
    tensors of 1 + n // hop_length frames each.  Nothing here waits for the device."""
    rms_dev = ctx.frame_rms(mix_dev, RMS_FRAME, int(hop_length))
    cen_dev, bw_dev = ctx.stft2048_centroid_bandwidth(mix_dev, sr, int(hop_length))
    return rms_dev, cen_dev, bw_dev


def _beats_from_device(ctx: "_native.Context", mix_dev, sr: int, hop_length: int) -> Tuple[float, np.ndarray]:
    """librosa.beat.beat_track(y=mix) on the device -> (tempo, beat times in seconds)."""
    from .rhythm import beat_track_from_device
    _, mel = ctx.stft2048_features(mix_dev, int(hop_length), want_flat=False, want_mel=True)
    env_dev = ctx.onset_strength(mel, int(hop_length), "median")
    del mel
    tempo, beats, _ = beat_track_from_device(ctx, env_dev, sr, int(hop_length))
    return float(tempo), (np.asarray(beats) * int(hop_length)).astype(int) / float(sr)


def _analyze(ctx: "_native.Context", mix_dev, series, n_samples: int, sr: int, hop_length: int, time_signature: int,
             energy_percentile: float, feature_cache) -> BeatAnalysisResult:
    audio_duration = n_samples / float(sr)
    beat_times: Optional[np.ndarray] = None
    tempo = 0.0
    if feature_cache is not None:
        cached = getattr(feature_cache, "beat_times", None)
        if cached is not None and len(cached) > 0:
            beat_times = cached
        bpm = getattr(feature_cache, "bpm_features", None)
        if bpm is not None:
            tempo = float(bpm.main_bpm)
    if beat_times is None:
        tempo, beat_times = _beats_from_device(ctx, mix_dev, sr, hop_length)
    elif tempo == 0.0 and len(beat_times) >= 2:
        spacing = float(np.mean(np.diff(beat_times)))
        tempo = 60.0 / spacing if spacing > 0 else DEFAULT_BPM
    if tempo == 0.0:
        tempo = DEFAULT_BPM
        logger.warning("[BeatAnalyzer] no tempo detected, using %.0f BPM", DEFAULT_BPM)
    bar_duration = 60.0 / tempo * time_signature
    bar_times = _generate_bar_boundaries(beat_times, audio_duration, time_signature)

    rms_dev, cen_dev, bw_dev = series
    n_bars = max(0, len(bar_times) - 1)
    if n_bars:
        lo, hi = bar_frame_ranges(frame_times(int(rms_dev.numel()), sr, hop_length), bar_times)
        means = ctx.bar_means3(rms_dev, cen_dev, bw_dev, lo, hi)
    else:
        means = np.zeros((3, 0), dtype=np.float64)
    bar_energies = [float(v) for v in means[0]]
    energy_threshold = float(np.percentile(bar_energies, energy_percentile)) if bar_energies else 0.0
    high = {i for i, e in enumerate(bar_energies) if e >= energy_threshold}
    logger.info("[BeatAnalyzer] BPM=%.1f, %d beats, %d bars, %d high-energy (P%.0f=%.4f)", tempo, len(beat_times), n_bars,
                len(high), energy_percentile, energy_threshold)
    return BeatAnalysisResult(tempo=tempo, beat_times=beat_times, bar_times=bar_times, bar_duration=bar_duration,
                              bar_energies=bar_energies, bar_spectral_centroids=[float(v) for v in means[1]],
                              bar_spectral_bandwidths=[float(v) for v in means[2]], high_energy_bars=high,
                              energy_threshold=energy_threshold)


def analyze_beats(audio: np.ndarray, sr: int, *, hop_length: int = 512, time_signature: int = 4, energy_percentile: float = 70.0,
                  feature_cache: Optional["TrackFeatureCache"] = None, ctx: Optional["_native.Context"] = None,
                  audio_dev=None, frame_series=None) -> BeatAnalysisResult:
    """Tempo, bars and per-bar features of `audio` (mono, or (2, N): its channel mean).  Beats and BPM are taken from
    `feature_cache` when it has them, else tracked on the device.  `audio_dev`: the track already on `ctx`'s device;
    `frame_series`: what `queue_frame_series` returned for that very mix at `hop_length`, when the caller queued it earlier."""
    audio = np.asarray(audio)
    n_samples = int(audio.shape[-1]) if audio.ndim == 2 else int(audio.size)
    if n_samples == 0:
        raise ValueError("analyze_beats needs a non-empty track")
    if ctx is None:
        ctx = _native.Context()
    mix_dev = _mono_on_device(ctx, _ensure_mono(audio) if audio_dev is None else audio, audio_dev)
    series = frame_series if frame_series is not None else queue_frame_series(ctx, mix_dev, sr, hop_length)   # ahead of any decision
    return _analyze(ctx, mix_dev, series, n_samples, int(sr), int(hop_length), int(time_signature), float(energy_percentile),
                    feature_cache)


class BeatAnalyzer:
    """`analyze_beats` with defaults kept on the instance and the last result remembered."""

    def __init__(self, sample_rate: int = 44100, hop_length: int = 512, time_signature: int = 4, energy_percentile: float = 70.0,
                 ctx: Optional["_native.Context"] = None):
        self.sample_rate = sample_rate
        self.hop_length = hop_length
        self.time_signature = time_signature
        self.energy_percentile = energy_percentile
        self.ctx = ctx
        self._last_result: Optional[BeatAnalysisResult] = None

    def analyze(self, audio: np.ndarray, *, sr: Optional[int] = None, hop_length: Optional[int] = None,
                time_signature: Optional[int] = None, energy_percentile: Optional[float] = None,
                feature_cache: Optional["TrackFeatureCache"] = None, ctx: Optional["_native.Context"] = None,
                audio_dev=None, frame_series=None) -> BeatAnalysisResult:
        if ctx is None:
            if self.ctx is None:
                self.ctx = _native.Context()
            ctx = self.ctx
        result = analyze_beats(audio, sr or self.sample_rate, hop_length=hop_length or self.hop_length,
                               time_signature=time_signature or self.time_signature,
                               energy_percentile=energy_percentile or self.energy_percentile, feature_cache=feature_cache,
                               ctx=ctx, audio_dev=audio_dev, frame_series=frame_series)
        self._last_result = result
        return result

    @property
    def last_result(self) -> Optional[BeatAnalysisResult]:
        return self._last_result


__all__ = ["BeatAnalysisResult", "BeatAnalyzer", "analyze_beats", "queue_frame_series", "bar_frame_ranges", "frame_times"]
