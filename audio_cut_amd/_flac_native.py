"""ctypes binding of libaudiocut_flac.so (include/flac/audiocut_flac.h): FLAC frames encoded on the device from the finished PCM
bytes that the packing kernels leave there.

A library, a header, a registry row and a binding class of their own, next to `_native` (whose `Context` lends the device, the
stream and `to_device`): nothing here is opened or imported unless `output.format` is `flac` (`utils/audio_export.py`).  There is
no CPU fallback behind these wrappers: a missing library or a failing call raises `NativeError`.  The host statement of the
encoder, which these kernels reproduce byte for byte, is `utils/flac_export.flac_encode_host`."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native import AbiSurface, NativeError
from .utils import flac_export as FX

_LIB_NAME = "libaudiocut_flac.so"
_lib: Optional[C.CDLL] = None

_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64

# include/flac/audiocut_flac.h; tests/test_flac_export_host.py holds this row against the header, type by type
FLAC_SURFACE = AbiSurface("flac/audiocut_flac.h", "acl_abi_version", 1, {
    "acl_abi_version": (_I, []),
    "acl_last_error": (C.c_char_p, []),
    "acl_flac_plan": (_I, [_P, _I64, _I, _I, _P, _I, _I, _P, _P, _P]),
    "acl_flac_write": (_I, [_P, _I64, _I, _I, _P, _I, _I, _I, _P, _P, _P, _I64, _P]),
})

RECORD_INTS = 160       # ACL_RECORD_INTS


def library_path() -> Path:
    return Path(__file__).resolve().parent / _LIB_NAME


def load() -> C.CDLL:
    """Load the FLAC library (built in-tree by `make -C audio_cut_amd/csrc`, whose `all` target builds all three libraries)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise NativeError(f"{path} is missing: build it with `make -C audio_cut_amd/csrc` (or `make -C audio_cut_amd/csrc/flac`); "
                          f"there is no CPU fallback for FLAC export of a device track")
    lib = C.CDLL(str(path))
    for name, (res, args) in FLAC_SURFACE.signatures.items():
        fn = getattr(lib, name)         # AttributeError here = the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    found = getattr(lib, FLAC_SURFACE.version_fn)()
    if found != FLAC_SURFACE.version:
        raise NativeError(f"{_LIB_NAME}: include/{FLAC_SURFACE.header} is at ABI version {found}, this binding expects "
                          f"{FLAC_SURFACE.version}; rebuild it with `make -C audio_cut_amd/csrc`")
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load().acl_last_error()
        raise NativeError(f"libaudiocut_flac call failed ({rc}): {msg.decode() if msg else '?'}")


class FlacKernels:
    """Typed wrappers over libaudiocut_flac.so for the device of a `_native.Context`."""

    def __init__(self, hip: "_native.Context"):
        self.hip = hip
        self.device = hip.device
        self.lib = load()
        self.last_ms: Optional[Tuple[float, float]] = None      # (plan, write) between device events, when `timed`
        self.timed = False

    def encode_device(self, pcm_dev: torch.Tensor, n_frames: int, channels: int, width: int, sample_rate: int, spans,
                      block_size: int) -> Tuple[torch.Tensor, List[Tuple[int, int, int, int]]]:
        """The frames of one FLAC file per span of the interleaved little-endian PCM bytes `pcm_dev` (uint8
        [n_frames * channels * width] on the device) -> (stream, files): the device byte stream, file after file, and each
        file's (offset, length, smallest frame, largest frame) in it; `flac_export.flac_header` goes in front of a file's bytes.
        Two launches (`acl_flac_plan`, `acl_flac_write`) with one small download between them: the frames' exact lengths, whose
        exclusive scan gives the offsets.  Spans may overlap; each is non-empty and inside [0, n_frames]."""
        n_frames, channels, width = int(n_frames), int(channels), int(width)
        if width not in (2, 3):
            raise ValueError(f"FLAC frames are made of 2-byte (PCM_16) or 3-byte (PCM_24) words, not {width}-byte ones")
        if channels not in (1, 2):
            raise ValueError(f"channels must be 1 or 2, got {channels}")
        block_size = FX.checked_block_size(block_size)
        code = FX.rate_code(FX.checked_rate(sample_rate))
        if n_frames <= 0:
            raise ValueError("encode: empty track")
        if (not isinstance(pcm_dev, torch.Tensor) or pcm_dev.dtype != torch.uint8 or pcm_dev.device != self.device or pcm_dev.dim() != 1
                or not pcm_dev.is_contiguous() or pcm_dev.numel() != n_frames * channels * width):
            raise NativeError(f"encode: expected a contiguous uint8 tensor of {n_frames * channels * width} bytes on the context's device")
        sp = FX.checked_spans(spans, n_frames)
        table = FX.frame_table(sp, block_size)
        rows = int(table.shape[0])
        d_table = self.hip.to_device(table)
        records = torch.empty((rows, RECORD_INTS), dtype=torch.int32, device=self.device)
        lengths = torch.empty(rows, dtype=torch.int32, device=self.device)
        events = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.timed else None
        if events:
            events[0].record()
        _check(self.lib.acl_flac_plan(pcm_dev.data_ptr(), n_frames, channels, width, d_table.data_ptr(), rows, block_size,
                                      records.data_ptr(), lengths.data_ptr(), _native._stream()))
        if events:
            events[1].record()
        lens = lengths.cpu().numpy().astype(np.int64)
        if (lens <= 0).any():
            raise NativeError("acl_flac_plan left a frame without bytes")
        offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        total = int(lens.sum())
        stream = torch.empty(total, dtype=torch.uint8, device=self.device)
        d_offsets = self.hip.to_device(offsets)
        if events:
            events[2].record()
        _check(self.lib.acl_flac_write(pcm_dev.data_ptr(), n_frames, channels, width, d_table.data_ptr(), rows, block_size, code,
                                       records.data_ptr(), d_offsets.data_ptr(), stream.data_ptr(), total, _native._stream()))
        if events:
            events[3].record()
            events[3].synchronize()
            self.last_ms = (events[0].elapsed_time(events[1]), events[2].elapsed_time(events[3]))
        files = []
        for f in range(sp.shape[0]):
            mine = np.flatnonzero(table[:, 0] == f)
            files.append((int(offsets[mine[0]]), int(lens[mine].sum()), int(lens[mine].min()), int(lens[mine].max())))
        return stream, files

    def encode(self, pcm_dev: torch.Tensor, n_frames: int, channels: int, width: int, sample_rate: int, spans, block_size: int,
               md5: bool = False) -> List[bytes]:
        """`encode_device`, one download of the stream, and the header in front of every file: `flac_encode_host` byte for byte.
        `md5`: the PCM bytes are downloaded too and every file's slice of them is hashed on the host."""
        import hashlib
        stream, files = self.encode_device(pcm_dev, n_frames, channels, width, sample_rate, spans, block_size)
        data = stream.cpu().numpy()
        raw = pcm_dev.cpu().numpy() if md5 else None
        stride = int(channels) * int(width)
        out = []
        for (lo, hi), (off, length, smallest, largest) in zip(FX.checked_spans(spans, n_frames), files):
            digest = hashlib.md5(raw[int(lo) * stride: int(hi) * stride].tobytes()).digest() if md5 else None
            out.append(FX.flac_header(sample_rate, int(channels), 8 * int(width), int(hi - lo), block_size, smallest, largest, digest)
                       + data[off: off + length].tobytes())
        return out


__all__ = ["FLAC_SURFACE", "FlacKernels", "library_path", "load"]
