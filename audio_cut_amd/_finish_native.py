"""ctypes binding of libaudiocut_finish.so (include/finish/audiocut_finish.h): segment fades and per-segment gains where the
resident float32 track becomes sample bytes.

A library, a header, a registry row and a binding class of their own, next to `_native` (whose `Context` lends the device, the
stream and `to_device`): nothing here is opened or imported unless segment finishing is switched on
(`utils/segment_finish.py`).  There is no CPU fallback behind these wrappers: a missing library or a failing call raises
`NativeError`."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._native import AbiSurface, NativeError
from .utils.audio_export import subtype_info

_LIB_NAME = "libaudiocut_finish.so"
_lib: Optional[C.CDLL] = None

_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64

# include/finish/audiocut_finish.h; tests/test_segment_finish_host.py holds this row against the header, type by type
FINISH_SURFACE = AbiSurface("finish/audiocut_finish.h", "acf_abi_version", 1, {
    "acf_abi_version": (_I, []),
    "acf_last_error": (C.c_char_p, []),
    "acf_span_stats": (_I, [_P, _I64, _I, _I64, _P, _P, _I, _I64, _I64, _P, _P, _P]),
    "acf_pack_spans": (_I, [_P, _I64, _I, _I64, _P, _P, _P, _I, _I64, _I64, _I, _P, _P]),
})

PARTS = 16      # partials per span of acf_span_stats


def library_path() -> Path:
    return Path(__file__).resolve().parent / _LIB_NAME


def load() -> C.CDLL:
    """Load the finish library (built in-tree by `make -C audio_cut_amd/csrc`, whose first target builds both libraries)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise NativeError(f"{path} is missing: build it with `make -C audio_cut_amd/csrc` (or `make -C audio_cut_amd/csrc/finish`); "
                          f"there is no CPU fallback for segment finishing on a device track")
    lib = C.CDLL(str(path))
    for name, (res, args) in FINISH_SURFACE.signatures.items():
        fn = getattr(lib, name)         # AttributeError here = the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    found = getattr(lib, FINISH_SURFACE.version_fn)()
    if found != FINISH_SURFACE.version:
        raise NativeError(f"{_LIB_NAME}: include/{FINISH_SURFACE.header} is at ABI version {found}, this binding expects "
                          f"{FINISH_SURFACE.version}; rebuild it with `make -C audio_cut_amd/csrc`")
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load().acf_last_error()
        raise NativeError(f"libaudiocut_finish call failed ({rc}): {msg.decode() if msg else '?'}")


def checked_spans(spans, n_frames: int) -> Tuple[np.ndarray, np.ndarray]:
    """(starts, ends) int64 of spans that are what the kernels are promised: at least one, each non-empty, inside [0, n_frames],
    sorted and disjoint.  Anything else is refused here, on the host, before a launch."""
    arr = np.asarray(list(spans), dtype=np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] == 0:
        raise ValueError(f"spans must be a non-empty list of (start, end) pairs, got shape {arr.shape}")
    a, b = np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1])
    if (b <= a).any():
        k = int(np.flatnonzero(b <= a)[0])
        raise ValueError(f"span {k} [{a[k]}, {b[k]}) is empty")
    if a[0] < 0 or b[-1] > int(n_frames) or (a < 0).any() or (b > int(n_frames)).any():
        raise ValueError(f"spans must lie inside [0, {int(n_frames)}]")
    if (a[1:] < b[:-1]).any():
        k = int(np.flatnonzero(a[1:] < b[:-1])[0]) + 1
        raise ValueError(f"spans must be sorted and must not overlap: span {k} starts at {a[k]}, span {k - 1} ends at {b[k - 1]}")
    return a, b


def _checked_fades(fade_in, fade_out) -> Tuple[int, int]:
    fi, fo = int(fade_in), int(fade_out)
    if fi != fade_in or fo != fade_out or fi < 0 or fo < 0:
        raise ValueError(f"fades are whole, non-negative frame counts, got {fade_in!r} and {fade_out!r}")
    return fi, fo


class FinishKernels:
    """Typed wrappers over libaudiocut_finish.so for the device of a `_native.Context`."""

    def __init__(self, hip: "_native.Context"):
        self.hip = hip
        self.device = hip.device
        self.lib = load()

    def _track(self, name: str, x: torch.Tensor) -> Tuple[int, int, int]:
        """(n_frames, channels, row stride) of a mono [n] or planar stereo [2, n] float32 track on the device, as `Context.pack_pcm`
        takes it: the rows of a stereo track may be views into wider rows."""
        if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.device or x.dim() not in (1, 2)
                or (x.dim() == 2 and x.shape[0] != 2)):
            raise NativeError(f"{name}: expected a float32 [n] or [2, n] tensor on the context's device")
        n, ch = int(x.shape[-1]), x.dim()
        if n == 0:
            raise NativeError(f"{name}: empty track")
        if x.stride(-1) != 1 or (ch == 2 and x.stride(0) < n):
            raise NativeError(f"{name}: the samples of a row must be contiguous and the rows must not overlap")
        return n, ch, int(x.stride(0)) if ch == 2 else n

    def span_stats(self, x_dev: torch.Tensor, spans, fade_in: int, fade_out: int) -> Tuple[np.ndarray, np.ndarray]:
        """(sumsq [n_spans] float64, peak [n_spans] float32) of the FADED samples of every span, all channels together: one launch
        of `acf_span_stats`, one download of the 16 partials per span, added and maxed in order on the host."""
        n, ch, stride = self._track("span_stats", x_dev)
        a, b = checked_spans(spans, n)
        fi, fo = _checked_fades(fade_in, fade_out)
        k = int(a.size)
        da, db = self.hip.to_device(a), self.hip.to_device(b)
        ss = torch.empty((k, PARTS), dtype=torch.float64, device=self.device)
        pk = torch.empty((k, PARTS), dtype=torch.float32, device=self.device)
        _check(self.lib.acf_span_stats(x_dev.data_ptr(), n, ch, stride, da.data_ptr(), db.data_ptr(), k, fi, fo, ss.data_ptr(),
                                       pk.data_ptr(), _native._stream()))
        parts = ss.cpu().numpy()
        total = np.zeros(k, dtype=np.float64)
        for p in range(PARTS):                      # fixed order: deterministic
            total += parts[:, p]
        return total, pk.cpu().numpy().max(axis=1)

    def pack_spans_device(self, x_dev: torch.Tensor, spans, gains, fade_in: int, fade_out: int, subtype: str,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The whole track as finished sample bytes of `subtype` on the device (uint8 [n * channels * width], stereo frames
        interleaved L, R): inside span k faded at both ends and multiplied by `gains[k]`, outside every span what
        `Context.pack_pcm_device` writes.  One launch of `acf_pack_spans`.  `out`: as for `pack_pcm_device`."""
        code, width = subtype_info(subtype)
        n, ch, stride = self._track("pack_spans", x_dev)
        a, b = checked_spans(spans, n)
        fi, fo = _checked_fades(fade_in, fade_out)
        g = np.asarray(gains)
        if g.dtype != np.float32 or g.shape != (a.size,):
            raise ValueError(f"pack_spans: gains must be a float32 array with one gain per span ({a.size}), got {g.dtype} {g.shape}")
        n_bytes = n * ch * width
        if out is None:
            out = torch.empty(n_bytes, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or out.dim() != 1 or out.numel() < n_bytes or not out.is_contiguous():
            raise NativeError(f"pack_spans: `out` must be a contiguous uint8 tensor of at least {n_bytes} bytes on the context's device")
        da, db, dg = self.hip.to_device(a), self.hip.to_device(b), self.hip.to_device(g)
        _check(self.lib.acf_pack_spans(x_dev.data_ptr(), n, ch, stride, da.data_ptr(), db.data_ptr(), dg.data_ptr(), int(a.size), fi, fo,
                                       code, out.data_ptr(), _native._stream()))
        return out[:n_bytes]

    def pack_spans(self, x_dev: torch.Tensor, spans, gains, fade_in: int, fade_out: int, subtype: str) -> np.ndarray:
        """`pack_spans_device` and one download: `pcm_bytes_host(finish_host(...))` (utils/segment_finish.py) bit for bit."""
        return self.pack_spans_device(x_dev, spans, gains, fade_in, fade_out, subtype).cpu().numpy()


__all__ = ["FINISH_SURFACE", "FinishKernels", "checked_spans", "library_path", "load"]
