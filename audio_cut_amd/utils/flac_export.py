"""FLAC export: the host statement of the encoder whose frames the device writes (`include/flac/audiocut_flac.h`, the stream's
specification; `_flac_native.FlacKernels`), the STREAMINFO header, the frame table and the three `output.flac` settings.

The encoder's input is not the float track: it is the finished, interleaved, little-endian PCM bytes the packing kernels leave
on the device, so a FLAC file decodes to exactly the integer samples the WAV of the same subtype holds.  Everything here is
integer arithmetic, so `flac_encode_host` and the kernels agree to the bit; the rules (stated once, here, and reproduced by
`csrc/flac/ac_flac.hip`):

  signals   mono: the channel.  Stereo: L, R, mid = (L + R) >> 1, side = L - R (one bit wider).
  constant  all samples of the frame equal: 8 + bps bits.
  fixed     orders 0..min(4, block - 1); partition orders 0..pmax, pmax = log2(block_size / 64) for a full block and 0 for a
            shorter last one.  u = fold(residual).  Per partition of n residuals with the sum S of u: k = the smallest k with
            (n << k) >= S (never above 30).  Estimate of (order, p) = order * bps + 4 * 2^p + sum over partitions of
            n * (k + 1) + (S >> k); the smallest estimate wins, ties to the smaller order, then the smaller p.  The winner's
            bits are then counted exactly; 5-bit parameters (method 01) if one of its k exceeds 14.
  verbatim  whenever the fixed subframe's exact count is not smaller than 8 + bps * block.
  stereo    the fewest exact bits among L/R, left/side, side/right, mid/side; ties to the earlier.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

FLAC_SUBTYPES: Dict[str, int] = {"PCM_16": 2, "PCM_24": 3}          # subtype -> bytes per word
BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
MAX_RATE = (1 << 20) - 1
MAX_FRAMES = 1 << 21
FINE = 64                                                           # samples of the finest partition of a full block
_RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
# channel assignment code -> the two candidate signals (0 L, 1 R, 2 mid, 3 side) in subframe order
ASSIGNMENTS = ((1, (0, 1)), (8, (0, 3)), (9, (3, 1)), (10, (2, 3)))


def _crc_table(poly: int, bits: int) -> List[int]:
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    table = []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data: bytes) -> int:
    """Polynomial 0x07, initial value 0, no reflection: the frame header's check."""
    c = 0
    for b in bytes(data):
        c = _CRC8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    """Polynomial 0x8005, initial value 0, no reflection: the frame's check."""
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def rate_code(sample_rate: int) -> int:
    return _RATE_CODES.get(int(sample_rate), 0)


def flac_subtype_width(subtype) -> int:
    """Bytes per word of a FLAC subtype; every other name is refused by name."""
    width = FLAC_SUBTYPES.get(subtype) if isinstance(subtype, str) else None
    if width is None:
        raise ValueError(f"unsupported FLAC subtype {subtype!r}: output.flac.subtype is one of {', '.join(FLAC_SUBTYPES)}")
    return width


def checked_block_size(block_size) -> int:
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or int(block_size) not in BLOCK_SIZES:
        raise ValueError(f"unsupported output.flac.block_size {block_size!r}: one of {', '.join(map(str, BLOCK_SIZES))}")
    return int(block_size)


def checked_rate(sample_rate) -> int:
    if int(sample_rate) <= 0 or int(sample_rate) > MAX_RATE:
        raise ValueError(f"sample rate {sample_rate} does not fit STREAMINFO's 20 bits (1..{MAX_RATE} Hz)")
    return int(sample_rate)


def checked_options(opts) -> Dict[str, object]:
    """{"subtype", "block_size", "md5"} of a FLAC options mapping, each refused by name if this build does not write it."""
    flac_subtype_width(opts.get("subtype"))
    md5 = opts.get("md5", False)
    if not isinstance(md5, (bool, np.bool_)):
        raise ValueError(f"unsupported output.flac.md5 {md5!r}: true or false")
    return {"subtype": str(opts["subtype"]), "block_size": checked_block_size(opts.get("block_size")), "md5": bool(md5)}


def configured_flac() -> Dict[str, object]:
    """`output.flac` over its defaults (`audio_export._DEFAULTS["flac"]`), read with `get_config` and checked (`checked_options`)."""
    from ..config import get_config
    from .audio_export import build_export_options
    return checked_options(build_export_options("flac", get_config("output.flac", {}) or {}))


def flac_header(sample_rate: int, channels: int, bits: int, total_samples: int, block_size: int, min_frame: int, max_frame: int,
                md5: Optional[bytes] = None) -> bytes:
    """`fLaC`, the one metadata block header and STREAMINFO: 42 bytes.  `md5` None: 16 zero bytes, "not computed"."""
    checked_rate(sample_rate)
    if channels not in (1, 2) or bits not in (16, 24) or not 0 <= total_samples < (1 << 36):
        raise ValueError(f"STREAMINFO cannot describe {channels} channel(s) of {bits} bits and {total_samples} samples")
    digest = bytes(16) if md5 is None else bytes(md5)
    if len(digest) != 16:
        raise ValueError("an MD5 signature has 16 bytes")
    packed = (int(sample_rate) << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | int(total_samples)
    return (b"fLaC" + bytes([0x80, 0, 0, 34]) + int(block_size).to_bytes(2, "big") * 2 + int(min_frame).to_bytes(3, "big")
            + int(max_frame).to_bytes(3, "big") + packed.to_bytes(8, "big") + digest)


def checked_spans(spans, n_frames: int) -> np.ndarray:
    """int64 [files, 2]: at least one span, each non-empty and inside [0, n_frames].  Spans may overlap: files are independent."""
    arr = np.asarray(list(spans), dtype=np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] == 0:
        raise ValueError(f"spans must be a non-empty list of (start, end) pairs, got shape {arr.shape}")
    if (arr[:, 1] <= arr[:, 0]).any():
        k = int(np.flatnonzero(arr[:, 1] <= arr[:, 0])[0])
        raise ValueError(f"span {k} [{arr[k, 0]}, {arr[k, 1]}) is empty")
    if (arr < 0).any() or (arr > int(n_frames)).any():
        raise ValueError(f"spans must lie inside [0, {int(n_frames)}]")
    return arr


def frame_table(spans, block_size: int) -> np.ndarray:
    """int64 [frames, 4]: (file index, frame number within the file, first sample of the track, block size) of every frame of every
    file, file after file.  A file of 2^21 or more frames is refused."""
    rows = []
    for f, (lo, hi) in enumerate(np.asarray(spans, dtype=np.int64).reshape(-1, 2)):
        count = -(-int(hi - lo) // block_size)
        if count >= MAX_FRAMES:
            raise ValueError(f"span {f} needs {count} frames of {block_size} samples; a file holds fewer than {MAX_FRAMES}")
        first = int(lo) + block_size * np.arange(count, dtype=np.int64)
        rows.append(np.stack([np.full(count, f, dtype=np.int64), np.arange(count, dtype=np.int64), first,
                              np.minimum(block_size, int(hi) - first)], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64)


def pcm_words(pcm_bytes, n_frames: int, channels: int, width: int) -> np.ndarray:
    """The interleaved little-endian PCM bytes as int64 [n_frames, channels]."""
    raw = np.frombuffer(pcm_bytes, dtype=np.uint8) if isinstance(pcm_bytes, (bytes, bytearray, memoryview)) \
        else np.asarray(pcm_bytes, dtype=np.uint8).reshape(-1)
    if width not in (2, 3) or channels not in (1, 2) or raw.size != n_frames * channels * width:
        raise ValueError(f"expected {n_frames * channels * width} bytes of {width}-byte words for {n_frames} frames of {channels} "
                         f"channel(s), got {raw.size}")
    b = raw.reshape(-1, width).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) if width == 2 else b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    sign = 1 << (8 * width - 1)
    return ((v ^ sign) - sign).reshape(n_frames, channels)


# ---- bits ------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self) -> None:
        self.parts: List[np.ndarray] = []

    def put(self, value: int, n: int) -> None:
        v = int(value) & ((1 << n) - 1)
        self.parts.append(np.array([(v >> (n - 1 - i)) & 1 for i in range(n)], dtype=np.uint8))

    def put_array(self, values: np.ndarray, n: int) -> None:
        v = np.asarray(values, dtype=np.int64) & ((1 << n) - 1)
        self.parts.append(((v[:, None] >> np.arange(n - 1, -1, -1, dtype=np.int64)) & 1).astype(np.uint8).reshape(-1))

    def put_rice(self, u: np.ndarray, k: int) -> None:
        """u >> k zero bits, a one bit, the low k bits of u, for every u."""
        q = u >> k
        length = q + 1 + k
        end = np.cumsum(length)
        bits = np.zeros(int(end[-1]) if u.size else 0, dtype=np.uint8)
        stop = end - k - 1
        bits[stop] = 1
        for b in range(k):
            bits[stop + 1 + b] = (u >> (k - 1 - b)) & 1
        self.parts.append(bits)

    def align(self) -> None:
        n = sum(p.size for p in self.parts)
        if n & 7:
            self.parts.append(np.zeros(8 - (n & 7), dtype=np.uint8))

    def tobytes(self) -> bytes:
        return np.packbits(np.concatenate(self.parts)).tobytes() if self.parts else b""


def _fold(r: np.ndarray) -> np.ndarray:
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _rice_k(n: np.ndarray, s: np.ndarray) -> np.ndarray:
    """The smallest k with (n << k) >= S, element by element."""
    k = np.zeros(n.shape, dtype=np.int64)
    for _ in range(30):
        k += ((n << k) < s).astype(np.int64)
    return k


def plan_subframe(s: np.ndarray, bps: int, block_size: int) -> Dict[str, object]:
    """The subframe chosen for the samples `s` (int64 [block]) of `bps` bits in a stream of block size `block_size`:
    {"type": "constant" | "verbatim" | "fixed", "bits": exact bits, and for fixed "order", "p", "k", "method"}."""
    bs = int(s.size)
    if (s == s[0]).all():
        return {"type": "constant", "bits": 8 + bps}
    verbatim = 8 + bps * bs
    pmax = (block_size // FINE).bit_length() - 1 if bs == block_size else 0
    best = None
    for order in range(min(4, bs - 1) + 1):
        u = np.concatenate([np.zeros(order, dtype=np.int64), _fold(np.diff(s, n=order))])
        for p in range(pmax + 1):
            n = np.full(1 << p, bs >> p, dtype=np.int64)
            n[0] -= order
            sums = u.reshape(1 << p, -1).sum(axis=1)
            k = _rice_k(n, sums)
            est = order * bps + 4 * (1 << p) + int(np.sum(n * (k + 1) + (sums >> k)))
            if best is None or est < best[0]:
                best = (est, order, p, k, u)
    _, order, p, k, u = best
    method = 1 if int(k.max()) > 14 else 0
    parts = u.reshape(1 << p, -1)
    bits = 8 + order * bps + 6 + (4 + method) * (1 << p)
    for q in range(1 << p):
        row = parts[q, order:] if q == 0 else parts[q]
        bits += int(np.sum((row >> k[q]) + 1 + k[q]))
    if bits >= verbatim:
        return {"type": "verbatim", "bits": verbatim}
    return {"type": "fixed", "bits": bits, "order": order, "p": p, "k": [int(v) for v in k], "method": method}


def _put_subframe(out: _Bits, s: np.ndarray, bps: int, plan: Dict[str, object]) -> None:
    if plan["type"] == "constant":
        out.put(0, 8)
        out.put(int(s[0]), bps)
    elif plan["type"] == "verbatim":
        out.put(1 << 1, 8)
        out.put_array(s, bps)
    else:
        order, p, k, method = int(plan["order"]), int(plan["p"]), plan["k"], int(plan["method"])
        out.put((8 | order) << 1, 8)
        if order:
            out.put_array(s[:order], bps)
        out.put(method, 2)
        out.put(p, 4)
        u = np.concatenate([np.zeros(order, dtype=np.int64), _fold(np.diff(s, n=order))]).reshape(1 << p, -1)
        for q in range(1 << p):
            out.put(k[q], 4 + method)
            out.put_rice(u[q, order:] if q == 0 else u[q], int(k[q]))


def _utf8_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    if v < 0x800:
        return bytes([0xC0 | (v >> 6), 0x80 | (v & 0x3F)])
    if v < 0x10000:
        return bytes([0xE0 | (v >> 12), 0x80 | ((v >> 6) & 0x3F), 0x80 | (v & 0x3F)])
    return bytes([0xF0 | (v >> 18), 0x80 | ((v >> 12) & 0x3F), 0x80 | ((v >> 6) & 0x3F), 0x80 | (v & 0x3F)])


def frame_header(frame_no: int, block: int, block_size: int, sample_rate: int, assignment: int, bits: int) -> bytes:
    """The frame header with its CRC-8; `assignment`: the 4-bit channel assignment code."""
    if block == block_size:
        size_code, tail = 8 + BLOCK_SIZES.index(block_size), b""
    elif block - 1 < 256:
        size_code, tail = 6, bytes([block - 1])
    else:
        size_code, tail = 7, (block - 1).to_bytes(2, "big")
    head = (bytes([0xFF, 0xF8, (size_code << 4) | rate_code(sample_rate), (assignment << 4) | ((4 if bits == 16 else 6) << 1)])
            + _utf8_number(frame_no) + tail)
    return head + bytes([crc8(head)])


def encode_frame(words: np.ndarray, bits: int, frame_no: int, block_size: int, sample_rate: int) -> bytes:
    """One frame from int64 [block, channels] words."""
    block, channels = words.shape
    if channels == 1:
        signals, widths = [words[:, 0]], [bits]
        plans = [plan_subframe(signals[0], bits, block_size)]
        code, pick = 0, (0,)
    else:
        left, right = words[:, 0], words[:, 1]
        signals, widths = [left, right, (left + right) >> 1, left - right], [bits, bits, bits, bits + 1]
        plans = [plan_subframe(sig, w, block_size) for sig, w in zip(signals, widths)]
        code, pick = min(ASSIGNMENTS, key=lambda a: sum(plans[c]["bits"] for c in a[1]))       # min keeps the first of equals
    out = _Bits()
    for c in pick:
        _put_subframe(out, signals[c], widths[c], plans[c])
    out.align()
    body = frame_header(frame_no, block, block_size, sample_rate, code, bits) + out.tobytes()
    return body + crc16(body).to_bytes(2, "big")


def assemble_file(frames: Sequence[bytes], n_samples: int, channels: int, bits: int, sample_rate: int, block_size: int,
                  md5: Optional[bytes] = None) -> bytes:
    sizes = [len(f) for f in frames]
    return flac_header(sample_rate, channels, bits, n_samples, block_size, min(sizes), max(sizes), md5) + b"".join(frames)


def flac_encode_host(pcm_bytes, n_frames: int, channels: int, width: int, sample_rate: int, spans, block_size: int,
                     md5: bool = False) -> List[bytes]:
    """One complete FLAC file per span of the interleaved little-endian PCM bytes of a track of `n_frames` frames: the statement
    the device encoder reproduces byte for byte, written one frame at a time."""
    block_size = checked_block_size(block_size)
    checked_rate(sample_rate)
    words = pcm_words(pcm_bytes, int(n_frames), int(channels), int(width))
    sp = checked_spans(spans, n_frames)
    table = frame_table(sp, block_size)
    raw = np.frombuffer(pcm_bytes, dtype=np.uint8) if isinstance(pcm_bytes, (bytes, bytearray, memoryview)) \
        else np.asarray(pcm_bytes, dtype=np.uint8).reshape(-1)
    files: List[bytes] = []
    for f, (lo, hi) in enumerate(sp):
        frames = [encode_frame(words[first: first + block], 8 * width, int(no), block_size, sample_rate)
                  for _, no, first, block in table[table[:, 0] == f]]
        stride = channels * width
        digest = hashlib.md5(raw[int(lo) * stride: int(hi) * stride].tobytes()).digest() if md5 else None
        files.append(assemble_file(frames, int(hi - lo), channels, 8 * width, sample_rate, block_size, digest))
    return files


__all__ = ["FLAC_SUBTYPES", "BLOCK_SIZES", "crc8", "crc16", "rate_code", "flac_subtype_width", "checked_block_size", "checked_rate",
           "checked_options", "configured_flac", "flac_header", "checked_spans", "frame_table", "pcm_words", "plan_subframe", "encode_frame",
           "assemble_file", "flac_encode_host"]
