"""Export at another sample rate: `output.sample_rate` ("Export rate").

The pipeline - detection, cuts, guards, the boundary policy - runs at `audio.sample_rate`; this module is what the export end needs
to let the files leave at another rate `R_out`, the input file's own (`"source"`) or a given one:

  * `resolve_output_rate(file_sr, sr)`: the configured value -> `R_out`, refusing what this build does not write;
  * `map_cut(c, sr, out_sr, n_out)`: a span end in pipeline samples -> the frame of the converted track it falls on;
  * `resample_pack_device(hip, x, up, down, subtype, n_out)`: the resident stem -> its finished sample bytes at the other rate in
    one launch (`ac_resample_poly_pack`, include/audiocut_hip_rate.h): `ac_resample_poly`'s floats through `ac_pack_pcm`'s
    conversion, with no float track at `R_out` in memory;
  * `resample_pack_host(x, up, down, subtype, n_out)`: the host statement of those bytes - the same taps, float64 sums rounded once
    to float32, `pcm_bytes_host` - for exporters that have no context and as the reference of the tests.

The reference has no such setting (it exports at the rate it loaded at), so the rules are stated here and pinned by
tests/test_output_rate_host.py and tests/test_output_rate_gpu.py.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import numpy as np

from .audio_export import pcm_bytes_host, subtype_info

# The ratio R_out / audio.sample_rate, reduced, may have no term above this: it admits 8, 11.025, 16, 22.05, 24, 32, 48, 88.2, 96,
# 176.4, 192 and 384 kHz against 44.1 kHz and keeps the designed low-pass at or below 245 k taps (`_resample_filter(1280, 147)`:
# 244 605).
MAX_RATIO_TERM = 1280


def rate_ratio(out_sr: int, sr: int) -> Tuple[int, int]:
    """(up, down) of sr -> out_sr, reduced by their greatest common divisor."""
    g = math.gcd(int(out_sr), int(sr))
    return int(out_sr) // g, int(sr) // g


def check_output_rate(value, sr: int, given=None) -> int:
    """`value` as an export rate against the pipeline rate `sr`, or ValueError naming it (`given`: the configured value it came
    from, when that is not the number itself).  Refused: anything but an int (a bool, a float and a string included), a rate
    <= 0, and a rate whose reduced ratio to `sr` has a term above MAX_RATIO_TERM."""
    shown = repr(value) if given is None else f"{given!r} (= {value!r})"
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"unsupported output.sample_rate {shown}: an integer rate in Hz, \"source\" or nothing")
    if int(value) <= 0:
        raise ValueError(f"unsupported output.sample_rate {shown}: the rate must be positive")
    up, down = rate_ratio(int(value), sr)
    if max(up, down) > MAX_RATIO_TERM:
        raise ValueError(f"unsupported output.sample_rate {shown}: its ratio to audio.sample_rate {sr} is {up}/{down}, and this build "
                         f"resamples by ratios whose terms are at most {MAX_RATIO_TERM}")
    return int(value)


def resolve_output_rate(file_sr: Optional[int], sr: int) -> int:
    """The rate of every exported file: `get_config("output.sample_rate", None)` resolved against the input file's rate `file_sr`
    (None: the input has none, a `.npy` array) and the pipeline rate `sr`.  Absent / None -> `sr`; "source" -> `file_sr` (`sr`
    without one); an integer -> that rate.  Every other value raises ValueError (`check_output_rate`)."""
    from ..config import get_config
    value = get_config("output.sample_rate", None)
    if value is None:
        return int(sr)
    if isinstance(value, str) and value == "source":
        return int(sr) if file_sr is None else check_output_rate(int(file_sr), sr, given=value)
    return check_output_rate(value, sr)


def resampled_len(n: int, up: int, down: int) -> int:
    """ceil(n * up / down): the frame count of a track of n frames after `ac_resample_poly`."""
    return -(-(int(n) * int(up)) // int(down))


def map_cut(c: int, sr: int, out_sr: int, n_out: int, n: Optional[int] = None) -> int:
    """A span end `c` in samples at `sr` -> its frame in the converted track of `n_out` frames at `out_sr`:
    min(n_out, (c * out_sr + sr // 2) // sr) in integers, i.e. c / sr seconds rounded to the nearest output frame.  0 maps to 0, the
    mapping is monotone, and with `n` (the track's length at `sr`) every c >= n maps to `n_out`: the end of the track is the end of
    the converted track, also where ceil(n * out_sr / sr) lies above the rounded value."""
    c = int(c)
    if n is not None and c >= int(n):
        return int(n_out)
    return max(0, min(int(n_out), (c * int(out_sr) + int(sr) // 2) // int(sr)))


@functools.lru_cache(maxsize=8)
def _host_rows(up: int, down: int):
    """(polyphase rows as float64 [up, tpp], n_pre_remove) of the shipped (up, down) low-pass: the taps `_resample_filter_dev`
    uploads."""
    from .._native import Context
    h, n_pre_remove = Context._resample_filter(up, down)
    return Context._polyphase_rows(h, up).astype(np.float64), int(n_pre_remove)


def _zero_sign(x64: np.ndarray, row: np.ndarray, j0: int) -> float:
    """The zero a sum of zero terms is in IEEE addition started at -0.0 (`ac_polyphase_dot_wave`): -0.0 only if every term of the
    (non-empty) tap range is -0.0; no term at all is +0.0."""
    n, tpp = x64.size, row.size
    t_lo, t_hi = max(0, j0 - (n - 1)), min(j0, tpp - 1)
    if t_lo > t_hi:
        return 0.0
    terms = row[t_lo: t_hi + 1] * x64[j0 - np.arange(t_lo, t_hi + 1)]
    return -0.0 if bool(np.all((terms == 0.0) & np.signbit(terms))) else 0.0


def resample_host(x: np.ndarray, up: int, down: int, n_out: int) -> np.ndarray:
    """One channel through the polyphase resampler on the host: y[m] = sum_t rows[p][t] x[j0 - t] with i = (m + n_pre_remove) down,
    j0 = i // up, p = i - j0 up over the samples of x only (tests/resample_refs.py `polyphase_ref64`'s definition, the shipped
    taps), every product and sum in float64, rounded once to float32.  m < n_out <= ceil(n up / down)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1)
    n = x64.size
    if not 1 <= int(n_out) <= resampled_len(n, up, down):
        raise ValueError(f"n_out {n_out} outside [1, {resampled_len(n, up, down)}] for {n} samples at {up}/{down}")
    rows, n_pre_remove = _host_rows(int(up), int(down))
    tpp = rows.shape[1]
    i = (np.arange(int(n_out), dtype=np.int64) + n_pre_remove) * int(down)
    j0 = i // int(up)
    p = i - j0 * int(up)
    # x zero-extended: tpp - 1 in front, and behind as far as the last j0 reaches; window k is x[k - tpp + 1 .. k], newest last
    xp = np.concatenate((np.zeros(tpp - 1), x64, np.zeros(max(0, int(j0[-1]) - (n - 1)))))
    win = np.lib.stride_tricks.sliding_window_view(xp, tpp)
    y = np.empty(int(n_out), dtype=np.float64)
    order = np.argsort(p, kind="stable")
    bounds = np.flatnonzero(np.diff(p[order])) + 1
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in np.split(order, bounds):
            taps = rows[int(p[idx[0]])][::-1]
            for k in range(0, idx.size, 32768):
                part = idx[k: k + 32768]
                y[part] = win[j0[part]] @ taps
        out = y.astype(np.float32)
    for m in np.flatnonzero(y == 0.0):
        out[m] = _zero_sign(x64, rows[int(p[m])], int(j0[m]))
    return out


def resample_pack_host(x: np.ndarray, up: int, down: int, subtype: str, n_out: int) -> np.ndarray:
    """The bytes `resample_pack_device` writes, stated on the host: each channel of the mono [n] or planar (2, n) track through
    `resample_host`, then `pcm_bytes_host` (stereo frames interleaved L, R).  uint8 [n_out * channels * width].  Equal rates
    after reduction: the first n_out frames converted as they are."""
    subtype_info(subtype)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[0] != 2):
        raise ValueError(f"expected a mono [n] or stereo (2, n) track, got shape {x.shape}")
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    if up == down == 1:
        y = x[..., : int(n_out)]
    else:
        y = np.stack([resample_host(ch, up, down, n_out) for ch in x]) if x.ndim == 2 else resample_host(x, up, down, n_out)
    return pcm_bytes_host(y.T if x.ndim == 2 else y, subtype)[0]


def resample_pack_device(hip, x, up: int, down: int, subtype: str, n_out: Optional[int] = None):
    """A mono [n] or planar stereo [2, n] float32 device track at fs -> its finished sample bytes of `subtype` at fs * up / down on
    the device (uint8 [n_out * channels * width], stereo frames interleaved L, R), one launch of `ac_resample_poly_pack`: every word
    is `hip.pack_pcm_device` of the float `hip.resample_poly` gives for its channel and index.  The rows of a stereo track may be
    views into wider rows.  `n_out`: the frames kept, 1 .. ceil(n up / down) (default: all); nothing is computed for the others.
    Equal rates after reduction have nothing to resample: `pack_pcm_device` of the first n_out frames."""
    import torch
    from .._native import NativeError, _check, _stream
    code, width = subtype_info(subtype)
    if x.dtype != torch.float32 or x.device != hip.device or x.dim() not in (1, 2) or (x.dim() == 2 and x.shape[0] != 2):
        raise NativeError("resample_pack: expected a float32 [n] or [2, n] tensor on the context's device")
    n, ch = int(x.shape[-1]), x.dim()
    if n == 0:
        raise NativeError("resample_pack: empty track")
    if x.stride(-1) != 1 or (ch == 2 and x.stride(0) < n):
        raise NativeError("resample_pack: the samples of a row must be contiguous and the rows must not overlap")
    up, down = hip._reduced_ratio(up, down)
    n_out = resampled_len(n, up, down) if n_out is None else int(n_out)
    if up == down == 1:
        if not 1 <= n_out <= n:
            raise NativeError(f"resample_pack: n_out {n_out} outside [1, {n}]")
        return hip.pack_pcm_device(x[..., :n_out], subtype)
    hd, n_pre_remove = hip._resample_filter_dev(up, down)
    out = torch.empty(max(n_out, 0) * ch * width, dtype=torch.uint8, device=hip.device)
    _check(hip.lib.ac_resample_poly_pack(hip._h, x.data_ptr(), n, ch, int(x.stride(0)) if ch == 2 else n, up, down, hd.data_ptr(),
                                         hd.numel(), n_pre_remove, code, out.data_ptr(), n_out, _stream()))
    return out


__all__ = ["MAX_RATIO_TERM", "rate_ratio", "check_output_rate", "resolve_output_rate", "resampled_len", "map_cut", "resample_host",
           "resample_pack_host", "resample_pack_device"]
