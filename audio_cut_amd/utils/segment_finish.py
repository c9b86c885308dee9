"""Segment finishing: a fade at each end of every exported segment and one gain per segment (RMS normalisation).

The reference ships the settings (`quality_control.fade_in_duration`, `fade_out_duration`, `normalize_audio`, `expert.yaml:105-107`)
and the arithmetic (`AudioProcessor.apply_fade`, `AudioProcessor.normalize_audio`; fade first, then normalise,
`quality_controller.py:750-757`) but never wires them into its export path.  Here they act on the segment files of a split: the
segments are byte ranges of one whole-track buffer, so the buffer is converted by a pack kernel that knows where the segments
are (`acf_pack_spans`, include/finish/audiocut_finish.h) after one small reduction for the gains (`acf_span_stats`).

The finished sample, for spans [s, e) of L frames, `Fi = int(fade_in_duration * sr)`, `Fo = int(fade_out_duration * sr)` and
i = f - s, every channel alike:
  1. fade in, only if Fi > 0 and L > Fi: for i < Fi, v = float32(float64(x) * linspace(0, 1, Fi)[i]);
  2. fade out, only if Fo > 0 and L > Fo: for i >= L - Fo, v = float32(float64(v) * linspace(1, 0, Fo)[i - (L - Fo)]);
  3. gain: y = v * g, one float32 product, g = 1 without normalisation;
  4. word: the conversion of the subtype (`pcm_bytes_host`).
The gain of a span: rms = sqrt(sumsq / (L * channels)) over the FADED samples in float64, g = float32(min(10 ** (target_db / 20) /
rms, max_gain)), 1.0 for a silent span or a sum that is not finite.  (The reference takes the RMS in float32 and its scalar
promotion depends on the numpy version; float64 sums and a float32 gain are this build's definition.)

`finish_host` is the host statement of steps 1-3 and the fallback for tracks that never were on the device; this module is
imported only when finishing is switched on."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from .audio_export import PackedTrack, _channels_of, pcm_bytes_host, subtype_info

INTEGER_SUBTYPES = ("PCM_U8", "PCM_16", "PCM_24", "PCM_32")


@dataclass(frozen=True)
class FinishSettings:
    fade_in_duration: float = 0.0
    fade_out_duration: float = 0.0
    normalize_audio: bool = False
    normalize_target_db: float = -20.0
    normalize_max_gain: float = 10.0
    fade_in_frames: int = 0
    fade_out_frames: int = 0

    @property
    def active(self) -> bool:
        return self.fade_in_frames > 0 or self.fade_out_frames > 0 or self.normalize_audio

    def as_dict(self) -> Dict[str, Any]:
        return {"fade_in_duration": self.fade_in_duration, "fade_out_duration": self.fade_out_duration,
                "normalize_audio": self.normalize_audio, "normalize_target_db": self.normalize_target_db,
                "normalize_max_gain": self.normalize_max_gain}


def _number(key: str, value) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"quality_control.{key} must be a number, got {value!r}")
    return float(value)


def finish_settings(values: Dict[str, Any], sr: int) -> FinishSettings:
    """The five keys of `quality_control` as settings; everything that cannot be honoured is refused by the key's name."""
    fades = {}
    for key in ("fade_in_duration", "fade_out_duration"):
        d = _number(key, values.get(key, 0.0))
        if not math.isfinite(d) or d < 0.0:
            raise ValueError(f"quality_control.{key} must be a finite duration of at least 0 seconds, got {d!r}")
        fades[key] = d
    target = _number("normalize_target_db", values.get("normalize_target_db", -20.0))
    if not math.isfinite(target):
        raise ValueError(f"quality_control.normalize_target_db must be finite, got {target!r}")
    max_gain = _number("normalize_max_gain", values.get("normalize_max_gain", 10.0))
    if not (max_gain > 0.0):
        raise ValueError(f"quality_control.normalize_max_gain must be greater than 0, got {max_gain!r}")
    norm = values.get("normalize_audio", False)
    if not isinstance(norm, (bool, np.bool_)):
        raise ValueError(f"quality_control.normalize_audio must be true or false, got {norm!r}")
    return FinishSettings(fades["fade_in_duration"], fades["fade_out_duration"], bool(norm), target, max_gain,
                          int(fades["fade_in_duration"] * sr), int(fades["fade_out_duration"] * sr))       # `apply_fade`: int(d * sr)


def configured_finish(sr: int) -> FinishSettings:
    from ..config import get_config
    keys = ("fade_in_duration", "fade_out_duration", "normalize_audio", "normalize_target_db", "normalize_max_gain")
    missing = object()
    values = {k: v for k in keys if (v := get_config(f"quality_control.{k}", missing)) is not missing and v is not None}
    return finish_settings(values, int(sr))


def gain_from_stats(sumsq, n_samples: int, settings: FinishSettings) -> np.float32:
    """The gain of a span from the float64 sum of squares of its `n_samples` faded samples (all channels)."""
    sumsq = float(sumsq)
    if not settings.normalize_audio or n_samples <= 0 or not math.isfinite(sumsq) or sumsq <= 0.0:
        return np.float32(1.0)
    rms = math.sqrt(sumsq / float(n_samples))
    if not (rms > 0.0) or not math.isfinite(rms):
        return np.float32(1.0)
    return np.float32(min(10.0 ** (settings.normalize_target_db / 20.0) / rms, settings.normalize_max_gain))


def _faded(piece: np.ndarray, fade_in: int, fade_out: int) -> np.ndarray:
    """Steps 1-2 on a copy of one span's samples [..., L] (float32), as `apply_fade` does them: in place, through float64."""
    piece = np.array(piece, dtype=np.float32)
    length = piece.shape[-1]
    if fade_in > 0 and length > fade_in:
        piece[..., :fade_in] *= np.linspace(0, 1, fade_in)
    if fade_out > 0 and length > fade_out:
        piece[..., length - fade_out:] *= np.linspace(1, 0, fade_out)
    return piece


def _spans(spans, n: int) -> List[Tuple[int, int]]:
    out = [(int(lo), int(hi)) for lo, hi in spans]
    last = 0
    for lo, hi in out:
        if lo < last or hi <= lo or hi > n:
            raise ValueError(f"spans must be non-empty, sorted, disjoint and inside [0, {n}]: [{lo}, {hi}) after {last}")
        last = hi
    return out


def finish_host(track: np.ndarray, spans, gains, fade_in: int, fade_out: int) -> np.ndarray:
    """Steps 1-3 in numpy: the float32 track (mono [N] or planar (2, N)) with every span faded and multiplied by its gain; frames
    outside the spans unchanged."""
    x = np.array(track, dtype=np.float32)
    _channels_of(x)
    g = np.asarray(gains, dtype=np.float32)
    sp = _spans(spans, x.shape[-1])
    if g.shape != (len(sp),):
        raise ValueError(f"one gain per span: {len(sp)} spans, gains of shape {g.shape}")
    for (lo, hi), gain in zip(sp, g):
        x[..., lo:hi] = _faded(x[..., lo:hi], int(fade_in), int(fade_out)) * gain
    return x


def finish_stats_host(track: np.ndarray, spans, fade_in: int, fade_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """(sumsq float64, peak float32) per span of the faded samples, all channels together; the sums by `math.fsum`."""
    x = np.asarray(track, dtype=np.float32)
    sp = _spans(spans, x.shape[-1])
    sumsq, peak = np.zeros(len(sp), dtype=np.float64), np.zeros(len(sp), dtype=np.float32)
    for k, (lo, hi) in enumerate(sp):
        v = _faded(x[..., lo:hi], int(fade_in), int(fade_out)).reshape(-1)
        sumsq[k] = math.fsum(np.square(v.astype(np.float64)).tolist())
        peak[k] = np.float32(np.fmax.reduce(np.abs(v), initial=np.float32(0.0)))
    return sumsq, peak


def finish_rows(sumsq, peak, gains, lengths: Sequence[int], channels: int, subtype: str) -> List[Dict[str, Any]]:
    """One dict per span: what was measured and what was applied."""
    rows = []
    for ss, pk, g, length in zip(sumsq, peak, gains, lengths):
        ms = float(ss) / float(length * channels) if (ss is not None and math.isfinite(float(ss))) else None
        g = float(np.float32(g))
        peak_out = None if pk is None else float(np.float32(pk) * np.float32(g))
        rows.append({
            "gain": g, "gain_db": 20.0 * math.log10(g) if g > 0.0 else None,
            "rms_db": None if ms is None else (10.0 * math.log10(ms) if ms > 0.0 else None),
            "peak_out": peak_out,
            "clipped": bool(subtype in INTEGER_SUBTYPES and peak_out is not None and peak_out >= 1.0),
        })
    return rows


def finished(audio, sample_rate: int, spans, settings: FinishSettings, subtype: str, *, hip=None, dev=None, flac=None) -> PackedTrack:
    """`PackedTrack.finished`: the whole track converted once, its spans finished.  With a context: the stats launch (only when
    normalising, else the gains are 1 and nothing is measured), the gains on the host, one launch of `acf_pack_spans`, one download.
    Without one: `finish_host` and `pcm_bytes_host`.  The track carries `finish_rows`.  `flac`: the FLAC form of the track
    (`PackedTrack`), whose finished bytes stay on the device."""
    subtype_info(subtype)
    channels = _channels_of(np.asarray(audio) if dev is None else dev)
    n = int(np.shape(audio)[-1])
    sp = _spans(spans, n)
    fi, fo = settings.fade_in_frames, settings.fade_out_frames
    lengths = [hi - lo for lo, hi in sp]
    sumsq: Sequence[Any] = [None] * len(sp)
    peak: Sequence[Any] = [None] * len(sp)
    gains = np.ones(len(sp), dtype=np.float32)
    if hip is not None:
        from .._finish_native import FinishKernels
        kernels = FinishKernels(hip)
        d = dev if dev is not None else hip.to_device(np.ascontiguousarray(audio, dtype=np.float32))
        if settings.normalize_audio:
            sumsq, peak = kernels.span_stats(d, sp, fi, fo)
            gains = np.array([gain_from_stats(ss, length * channels, settings) for ss, length in zip(sumsq, lengths)], dtype=np.float32)
        data = kernels.pack_spans(d, sp, gains, fi, fo, subtype) if flac is None else kernels.pack_spans_device(d, sp, gains, fi, fo, subtype)
    else:
        x = np.asarray(audio, dtype=np.float32)
        if settings.normalize_audio:
            sumsq, peak = finish_stats_host(x, sp, fi, fo)
            gains = np.array([gain_from_stats(ss, length * channels, settings) for ss, length in zip(sumsq, lengths)], dtype=np.float32)
        y = finish_host(x, sp, gains, fi, fo)
        data, _ = pcm_bytes_host(y.T if channels == 2 else y, subtype)
    track = PackedTrack.from_bytes(data, n, channels, int(sample_rate), subtype, flac=flac, hip=hip)
    track.finish_rows = finish_rows(sumsq, peak, gains, lengths, channels, subtype)
    return track


__all__ = ["FinishSettings", "finish_settings", "configured_finish", "gain_from_stats", "finish_host",
           "finish_stats_host", "finish_rows", "finished"]
