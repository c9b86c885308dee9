"""RIFF/WAVE reader of the loader: the header walk (`read_wav_info`) and the numpy statement of the sample arithmetic
(`decode_host`) that `ac_decode_pcm` (include/audiocut_hip_load.h) reproduces bit for bit on the device.

The standard library's `wave` reads format tag 1 alone.  This reader takes what `librosa.load` takes among uncompressed WAVs
(reference `src/vocal_smart_splitter/utils/audio_processor.py:45-49`): PCM (tag 1) of 8, 16, 24 and 32 bits, IEEE float (tag 3) of
32 and 64 bits, and both again as WAVE_FORMAT_EXTENSIBLE (tag 0xFFFE: ffmpeg writes it for every 24- and 32-bit file, most tools
for every file of more than two channels).  Samples are decoded by CONTAINER width (`block_align / channels`) and are left-justified
in it, as the WAV specification says and libsndfile reads them: 24 valid bits in a 4-byte container are a 32-bit sample.

Refused by class, with the cause in the message (`UnsupportedAudioError`, a `ValueError`): RF64 and RIFX containers, companded and
compressed tags (A-law, mu-law, ADPCM, MPEG, ...), an extensible sub-format GUID that is not KSDATAFORMAT's, a `block_align` that
does not fit channels x width, a missing `fmt ` or `data` chunk.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Union

import numpy as np


class UnsupportedAudioError(ValueError):
    """The file is not an uncompressed RIFF/WAVE this loader reads; the message names the cause."""


# sample_format -> (code of ac_decode_pcm's `sample_format`, container bytes): keep in step with include/audiocut_hip_load.h
SAMPLE_FORMATS = {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4), "f64": (5, 8)}
LAYOUT_MONO, LAYOUT_PLANAR = 0, 1
MAX_CHANNELS = 8

_TAG_PCM, _TAG_FLOAT, _TAG_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000AA00389B71")       # bytes 2..15 of KSDATAFORMAT_SUBTYPE_*
_TAG_NAMES = {0x0002: "MS ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10", 0x0040: "G.721 ADPCM",
              0x0050: "MPEG", 0x0055: "MPEG layer 3"}


@dataclass(frozen=True)
class WavInfo:
    sample_rate: int
    channels: int
    sample_format: str          # a key of SAMPLE_FORMATS
    container_bytes: int        # block_align / channels: the width the samples are decoded by
    bits_per_sample: int        # valid bits (<= 8 * container_bytes); informational
    n_frames: int
    data_offset: int            # of the first sample byte in the file
    data_bytes: int             # n_frames * channels * container_bytes (a trailing partial frame is dropped)

    @property
    def format_code(self) -> int:
        return SAMPLE_FORMATS[self.sample_format][0]


def _parse_fmt(body: bytes, where: str):
    """`fmt ` chunk body -> (sample_rate, channels, sample_format, container_bytes, bits_per_sample)."""
    if len(body) not in (16, 18, 40):
        raise UnsupportedAudioError(f"{where}: fmt chunk of {len(body)} bytes (16, 18 or 40 expected)")
    tag, channels, rate, _byte_rate, block_align, bits = struct.unpack_from("<HHIIHH", body, 0)
    valid_bits = bits
    if tag == _TAG_EXTENSIBLE:
        if len(body) != 40:
            raise UnsupportedAudioError(f"{where}: WAVE_FORMAT_EXTENSIBLE needs a 40-byte fmt chunk, this one has {len(body)}")
        _cb, valid, _mask = struct.unpack_from("<HHI", body, 16)
        guid = body[24:40]
        if guid[2:] != _KSDATAFORMAT_TAIL:
            raise UnsupportedAudioError(f"{where}: sub-format GUID mismatch ({guid.hex()} is not a KSDATAFORMAT sub-type)")
        tag = struct.unpack_from("<H", guid, 0)[0]
        valid_bits = valid or bits
    if tag not in (_TAG_PCM, _TAG_FLOAT):
        name = _TAG_NAMES.get(tag)
        raise UnsupportedAudioError(f"{where}: unsupported format tag 0x{tag:04X}" + (f" ({name})" if name else "")
                                    + ": only PCM (1) and IEEE float (3) are read")
    if not 1 <= channels <= MAX_CHANNELS:
        raise UnsupportedAudioError(f"{where}: {channels} channels (1 to {MAX_CHANNELS} are read)")
    if rate <= 0:
        raise UnsupportedAudioError(f"{where}: sample rate {rate}")
    width = block_align // channels
    allowed = {1: "u8", 2: "s16", 3: "s24", 4: "s32"} if tag == _TAG_PCM else {4: "f32", 8: "f64"}
    if block_align % channels or width not in allowed or not 0 < valid_bits <= 8 * width or bits > 8 * width:
        kind = "PCM" if tag == _TAG_PCM else "float"
        raise UnsupportedAudioError(f"{where}: inconsistent block_align {block_align} for {channels} channels of {bits}-bit {kind} "
                                    f"({'1, 2, 3 or 4' if tag == _TAG_PCM else '4 or 8'} bytes per sample expected)")
    return int(rate), int(channels), allowed[width], int(width), int(valid_bits)


def read_wav_info(path: Union[str, os.PathLike]) -> WavInfo:
    """Walk the RIFF chunks of `path`: the first `fmt ` and the first `data` chunk count, every other chunk (LIST, bext, JUNK, fact,
    ...) is skipped wherever it stands, odd sizes with their pad byte.  A `data` length of 0 or 0xFFFFFFFF, or one that runs past
    the end of the file (a writer that could not seek back, e.g. ffmpeg into a pipe), means the data run to the end of the file."""
    where = str(path)
    size = os.path.getsize(path)
    fmt = None
    data = None
    with open(path, "rb") as fh:
        head = fh.read(12)
        magic = head[:4]
        if magic == b"RF64":
            raise UnsupportedAudioError(f"{where}: RF64 container (64-bit RIFF) is not read")
        if magic == b"RIFX":
            raise UnsupportedAudioError(f"{where}: RIFX container (big-endian RIFF) is not read")
        if len(head) < 12 or magic != b"RIFF" or head[8:12] != b"WAVE":
            raise UnsupportedAudioError(f"{where}: not a RIFF/WAVE file")
        pos = 12
        while pos + 8 <= size and (fmt is None or data is None):
            fh.seek(pos)
            cid, csize = struct.unpack("<4sI", fh.read(8))
            body = pos + 8
            if cid == b"fmt " and fmt is None:
                fmt = _parse_fmt(fh.read(min(csize, 64)), where)
            elif cid == b"data" and data is None:
                if csize in (0, 0xFFFFFFFF) or body + csize > size:
                    data = (body, size - body)
                    break                                   # the data run to the end: no chunk can follow
                data = (body, csize)
            pos = body + csize + (csize & 1)
    if fmt is None:
        raise UnsupportedAudioError(f"{where}: no fmt chunk" + (" in front of the data that run to the end of the file" if data else ""))
    if data is None:
        raise UnsupportedAudioError(f"{where}: no data chunk")
    rate, channels, sample_format, width, bits = fmt
    n_frames = data[1] // (channels * width)
    if n_frames == 0:
        raise ValueError(f"{where}: the data chunk holds no whole frame")
    return WavInfo(sample_rate=rate, channels=channels, sample_format=sample_format, container_bytes=width, bits_per_sample=bits,
                   n_frames=int(n_frames), data_offset=int(data[0]), data_bytes=int(n_frames * channels * width))


def read_wav_bytes(path: Union[str, os.PathLike], info: WavInfo, into: np.ndarray = None) -> np.ndarray:
    """The `info.data_bytes` sample bytes of the file, read once: into `into` (a writable uint8 array of at least that length, e.g.
    pinned staging memory) or into a new array."""
    buf = np.empty(info.data_bytes, dtype=np.uint8) if into is None else into
    view = memoryview(buf)[: info.data_bytes]
    with open(path, "rb", buffering=0) as fh:
        fh.seek(info.data_offset)
        got = 0
        while got < info.data_bytes:
            k = fh.readinto(view[got:])
            if not k:
                raise ValueError(f"{path}: the file ended {info.data_bytes - got} bytes short of its data chunk")
            got += k
    return buf[: info.data_bytes]


def decode_samples(raw: np.ndarray, info: WavInfo) -> np.ndarray:
    """Interleaved sample bytes -> float32 [n_frames, channels].  16-, 24- and 32-bit PCM: the loader's arithmetic since its first
    version, kept bit for bit."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)[: info.data_bytes]
    if raw.size != info.data_bytes:
        raise ValueError(f"decode: {raw.size} bytes given, the header implies {info.data_bytes}")
    f = info.sample_format
    if f == "u8":
        data = (raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif f == "s16":
        data = raw.view("<i2").astype(np.float32) / 32768.0
    elif f == "s24":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        data = v.astype(np.float32) / 8388608.0
    elif f == "s32":
        data = raw.view("<i4").astype(np.float32) / 2147483648.0          # int32 -> float32 rounds to nearest even
    elif f == "f32":
        data = raw.view("<f4").astype(np.float32, copy=True)              # the bits as they are: nothing is clipped
    elif f == "f64":
        with np.errstate(over="ignore", invalid="ignore"):
            data = raw.view("<f8").astype(np.float32)                     # rounded once; beyond float32's range: +-inf
    else:
        raise ValueError(f"unknown sample format {f!r}")
    return data.reshape(-1, info.channels)


def channel_mean(data: np.ndarray) -> np.ndarray:
    """float32 [n, channels] -> float32 [n]: the float32 sum in channel order divided by float32(channels); one channel: a copy."""
    acc = data[:, 0].copy()
    if data.shape[1] == 1:
        return acc
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(1, data.shape[1]):
            acc = acc + data[:, c]
        return (acc / np.float32(data.shape[1])).astype(np.float32)


def decode_host(raw: np.ndarray, info: WavInfo, layout: int) -> np.ndarray:
    """What `ac_decode_pcm` computes, in numpy.  `LAYOUT_MONO`: float32 [n], the float32 sum of the channels in channel order
    divided by float32(channels) (one channel: the samples themselves) - what `np.mean(axis=1)` gives for up to six channels; at
    seven and eight numpy sums pairwise and this rule is the definition.  `LAYOUT_PLANAR`: float32 [channels, n]."""
    data = decode_samples(raw, info)
    if layout == LAYOUT_PLANAR:
        return np.ascontiguousarray(data.T)
    if layout != LAYOUT_MONO:
        raise ValueError(f"unknown layout {layout!r}")
    return channel_mean(data)


def count_nonfinite(raw: np.ndarray, info: WavInfo) -> int:
    """The number of samples whose float32 value is NaN or +-infinity (0 for the integer formats): `ac_decode_pcm`'s count."""
    if info.sample_format not in ("f32", "f64"):
        return 0
    return int(np.count_nonzero(~np.isfinite(decode_samples(raw, info))))


def read_wav(path: Union[str, os.PathLike]):
    """(float32 [n_frames, channels], sample_rate) on the host; a NaN or an infinity in a float file is refused, as the device
    loader and `librosa.load` (`valid_audio`) refuse it."""
    info = read_wav_info(path)
    data = decode_samples(read_wav_bytes(path, info), info)
    if info.sample_format in ("f32", "f64"):
        bad = int(np.count_nonzero(~np.isfinite(data)))
        if bad:
            raise ValueError(f"{Path(path)}: {bad} samples are NaN or infinite")
    return data, info.sample_rate


__all__ = ["UnsupportedAudioError", "WavInfo", "SAMPLE_FORMATS", "LAYOUT_MONO", "LAYOUT_PLANAR", "MAX_CHANNELS", "read_wav_info",
           "read_wav_bytes", "decode_samples", "channel_mean", "decode_host", "count_nonfinite", "read_wav"]
