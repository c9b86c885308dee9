"""Audio export — mirror of the reference's `src/vocal_smart_splitter/utils/audio_export.py` (`ensure_supported_format`,
`build_export_options`, `export_audio`) and `core/utils/segment_exporter.py` (`ExportResult`, `SegmentExporter`) for the
formats this build writes: WAV of the subtypes PCM_24 (the reference default, `audio_export.py:109-111`), PCM_U8, PCM_16, PCM_32,
FLOAT and DOUBLE (`output.wav.subtype`, what `soundfile.write(.., subtype=..)` gets there).  SURVEY.md §8(f) row 4.

The float -> integer conversion runs on the GPU (`ac_pack_pcm`, one kernel for all six subtypes) on the whole resident track once and is libsndfile's
clipping conversion - python-soundfile sets SFC_SET_CLIPPING on every file, so `soundfile.write` goes through pcm.c
`f2let_clip_array`: `lrintf(x * 2^31) >> 8`, saturating at 0x7FFFFF / 0x800000 (`>> 16` for PCM_16, `>> 24` plus 128 for PCM_U8, the
whole word for PCM_32); FLOAT is the float32 bits as they are and DOUBLE their exact widening, nothing clipped.  Segment files are
byte slices of that buffer behind a RIFF header (44 bytes for the integer subtypes, 56 with the `fact` chunk of the float ones).
MP3 needs pydub + FFmpeg in the reference (`:114-135`) and is refused here.
FLAC (`output.format: flac`, this build's own) is encoded from the same sample bytes - on the device when they are there - and
decodes to exactly the WAV's integer samples: `PackedTrack`'s FLAC form, `utils/flac_export.py`, `_flac_native.py`.
Stereo tracks are planar (2, N) arrays (the reference writes `(channels, samples)` arrays as multichannel files, `:93-106`): they
are interleaved frame by frame in the packing kernel, which reads the planar rows as they are, and the header carries two channels.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

# `output.<format>` defaults.  The FLAC ones live here, not in `config.DEFAULTS`: `output.flac.subtype` (PCM_16 or PCM_24),
# `output.flac.block_size` (256..4096) and `output.flac.md5` (`utils/flac_export.py`)
_DEFAULTS: Dict[str, Dict[str, object]] = {"wav": {"subtype": "PCM_24"}, "flac": {"subtype": "PCM_24", "block_size": 4096, "md5": False}}


# subtype -> (AC_PACK_* code of include/audiocut_hip_pack.h, bytes per word)
WAV_SUBTYPES: Dict[str, Tuple[int, int]] = {"PCM_U8": (0, 1), "PCM_16": (1, 2), "PCM_24": (2, 3), "PCM_32": (3, 4), "FLOAT": (4, 4),
                                            "DOUBLE": (5, 8)}


def subtype_info(subtype) -> Tuple[int, int]:
    """(kernel code, bytes per word) of a subtype name.  Every other name (ULAW, ALAW, the ADPCMs, PCM_S8, a misspelling) is refused."""
    info = WAV_SUBTYPES.get(subtype) if isinstance(subtype, str) else None
    if info is None:
        raise ValueError(f"unsupported WAV subtype {subtype!r}: this build writes {', '.join(WAV_SUBTYPES)}")
    return info


def ensure_supported_format(name: Optional[str]) -> str:
    key = (name or "wav").strip().lower()
    if key not in _DEFAULTS:
        raise ValueError(f"unsupported export format {name!r}: this build writes {sorted(_DEFAULTS)}")
    return key


def build_export_options(format_name: str, *overrides: Optional[Dict[str, object]]) -> Dict[str, object]:
    opts: Dict[str, object] = dict(_DEFAULTS[ensure_supported_format(format_name)])
    for o in overrides:
        if o:
            opts.update(o)
    return opts


def configured_subtype() -> str:
    """The WAV subtype the configuration asks for: `output.format` (refused unless this build writes it) and `output.<format>`
    over the format's defaults, as the reference's splitter reads them (`seamless_splitter.py:98-103,167-192`)."""
    from ..config import get_config
    fmt = ensure_supported_format(get_config("output.format", "wav"))
    if fmt == "flac":                       # FLAC's own two subtypes, block size and MD5 switch, each refused by name
        from .flac_export import configured_flac
        return str(configured_flac()["subtype"])
    subtype = build_export_options(fmt, get_config(f"output.{fmt}", {}) or {}).get("subtype", "PCM_24")
    subtype_info(subtype)
    return str(subtype)


def configured_flac_options() -> Optional[Dict[str, object]]:
    """The checked `output.flac` settings when `output.format` is `flac`, else None - and then nothing of FLAC is imported."""
    from ..config import get_config
    if ensure_supported_format(get_config("output.format", "wav")) != "flac":
        return None
    from .flac_export import configured_flac
    return configured_flac()


def _export_path(base_path: Path, ext: str) -> Path:
    """`export_audio` (`:70-90`): a base name that already contains a dot keeps it (durations like `_12.3`)."""
    base_path = Path(base_path)
    return base_path.parent / f"{base_path.name}.{ext}" if base_path.suffix else base_path.with_suffix(f".{ext}")


def wav_header(n_frames: int, sample_rate: int, channels: int, bytes_per_sample: int, subtype: Optional[str] = None) -> bytes:
    """Everything in front of the sample bytes.  Integer subtypes (`subtype` None: the integer one of that width): format tag 1,
    a 16-byte `fmt ` chunk, `data` - 44 bytes.  FLOAT and DOUBLE: tag 3, the same `fmt ` chunk, a `fact` chunk with the frame count,
    `data` - 56 bytes; no PEAK chunk (libsndfile's carries a timestamp).  A PCM_U8 data chunk of odd length is followed by one pad
    byte (`wav_pad`), which the RIFF size counts; PCM_24 files keep the layout they have always had here (no pad byte behind an
    odd number of mono samples), byte for byte, and no other subtype can be odd.  Sizes that do not fit the 32-bit fields are refused: RF64 is not written."""
    if subtype is not None and subtype_info(subtype)[1] != bytes_per_sample:
        raise ValueError(f"a {subtype} word has {subtype_info(subtype)[1]} bytes, not {bytes_per_sample}")
    is_float = subtype in ("FLOAT", "DOUBLE")
    data = n_frames * channels * bytes_per_sample
    riff = (48 if is_float else 36) + data + len(wav_pad(n_frames, channels, bytes_per_sample))
    if data > 0xFFFFFFFF or riff > 0xFFFFFFFF:
        raise ValueError(f"{data} sample bytes do not fit a RIFF/WAVE file (32-bit sizes); RF64 is not written")
    fact = b"fact" + struct.pack("<II", 4, n_frames) if is_float else b""
    return (b"RIFF" + struct.pack("<I", riff) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3 if is_float else 1, channels, sample_rate,
            sample_rate * channels * bytes_per_sample, channels * bytes_per_sample, 8 * bytes_per_sample) + fact + b"data" + struct.pack("<I", data))


def wav_pad(n_frames: int, channels: int, bytes_per_sample: int) -> bytes:
    """The RIFF pad byte behind a PCM_U8 data chunk of odd length, else nothing (see `wav_header` for PCM_24)."""
    return b"\0" if bytes_per_sample == 1 and (n_frames * channels) & 1 else b""


def _sndfile_clip_int32(x: np.ndarray) -> np.ndarray:
    """libsndfile pcm.c f2le{s,t}_clip_array (python-soundfile enables SFC_SET_CLIPPING on every file): the sample times 2^31
    in float32, saturated at 0x7FFFFFFF / -2^31, then lrintf (half to even).  The PCM word is its top 2 or 3 bytes."""
    s = np.asarray(x, dtype=np.float32) * np.float32(2147483648.0)
    v = np.rint(np.nan_to_num(s.astype(np.float64), nan=0.0, posinf=3e9, neginf=-3e9))
    v = np.where(s >= np.float32(2147483647.0), 2147483647.0, np.where(s <= np.float32(-2147483648.0), -2147483648.0, v))
    return v.astype(np.int64)


def pcm_bytes_host(audio: np.ndarray, subtype: str) -> Tuple[np.ndarray, int]:
    """Host conversion for arrays that never were on the device (tests, tiny inputs): same arithmetic as the kernels, which is
    libsndfile's clipping float -> PCM conversion: `lrintf(x * 2^31)` (PCM_32), `>> 8` (PCM_24), `>> 16` (PCM_16), `(>> 24) + 128`
    (PCM_U8); FLOAT is the float32 bits as they are (NaN and infinities kept) and DOUBLE their exact widening."""
    subtype_info(subtype)
    x = np.asarray(audio, dtype=np.float32).reshape(-1)
    if subtype == "FLOAT":
        return x.astype("<f4").view(np.uint8), 4
    if subtype == "DOUBLE":
        return x.astype("<f8").view(np.uint8), 8
    if subtype == "PCM_32":
        return _sndfile_clip_int32(x).astype("<i4").view(np.uint8), 4
    if subtype == "PCM_U8":
        return ((_sndfile_clip_int32(x) >> 24) + 128).astype(np.uint8), 1
    if subtype == "PCM_16":
        return (_sndfile_clip_int32(x) >> 16).astype("<i2").view(np.uint8), 2
    v = (_sndfile_clip_int32(x) >> 8).astype(np.int32)
    out = np.empty((x.size, 3), dtype=np.uint8)
    out[:, 0] = v & 0xFF; out[:, 1] = (v >> 8) & 0xFF; out[:, 2] = (v >> 16) & 0xFF
    return out.reshape(-1), 3


def _channels_of(audio) -> int:
    """1 for a mono [N] track, 2 for a planar stereo (2, N) one."""
    nd = len(audio.shape)
    if nd == 1:
        return 1
    if nd == 2 and audio.shape[0] == 2:
        return 2
    raise ValueError(f"this build exports mono [N] or stereo (2, N) tracks, got shape {tuple(audio.shape)}")


class PackedTrack:
    """A whole mono [N] or planar stereo (2, N) track converted once (on the GPU when a context and device tensor are given);
    slices are cheap.  Stereo frames are interleaved (L, R) like every multichannel WAV.  `subtype`: one of `WAV_SUBTYPES`.

    The FLAC form (`flac`: the checked settings of `flac_export.checked_options`, None for WAV): the same sample bytes, which
    with a context STAY a device tensor; `prepare(spans)` encodes the spans to be written in one `FlacKernels.encode` call (two
    launches, one download of the compressed stream; the PCM bytes are downloaded only for `md5`) and `write` emits the
    STREAMINFO header and that span's frames.  Without a context the bytes are host bytes and `flac_encode_host` encodes them."""

    flac: Optional[Dict[str, object]] = None
    hip = None

    def __init__(self, audio: np.ndarray, sample_rate: int, subtype: str = "PCM_24", *, hip=None, dev=None,
                 flac: Optional[Dict[str, object]] = None) -> None:
        subtype_info(subtype)
        if flac is not None:
            self._set_flac(flac, subtype, hip)
        self.sample_rate = int(sample_rate)
        self.subtype = subtype
        self.channels = _channels_of(np.asarray(audio) if dev is None else dev)
        self.n = int(np.shape(audio)[-1])
        if hip is not None and self.n > 0:                  # the planar track as it is, interleaved in the kernel
            d = dev if dev is not None else hip.to_device(np.ascontiguousarray(audio, dtype=np.float32))
            self.bytes = hip.pack_pcm(d, subtype) if flac is None else hip.pack_pcm_device(d, subtype)
            self.width = subtype_info(subtype)[1]
        else:
            x = np.asarray(audio)
            self.bytes, self.width = pcm_bytes_host(x.T if self.channels == 2 else x, subtype)

    @classmethod
    def from_bytes(cls, data, n: int, channels: int, sample_rate: int, subtype: str, *, flac: Optional[Dict[str, object]] = None,
                   hip=None) -> "PackedTrack":
        """Wrap sample bytes of `subtype` that are ready (`ac_mdx_assemble_pcm`): `width * channels * n` of them, stereo frames
        interleaved L, R - the layout the constructor produces.  The FLAC form with a context takes them as a uint8 device tensor."""
        width = subtype_info(subtype)[1]
        on_device = flac is not None and hip is not None and not isinstance(data, (bytes, bytearray, memoryview, np.ndarray))
        if on_device:
            data = data.reshape(-1)
            size = int(data.numel())
        else:
            data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, dtype=np.uint8).reshape(-1)
            size = int(data.size)
        if channels not in (1, 2) or n < 0 or size != width * channels * n:
            raise ValueError(f"expected {width * channels * n} {subtype} bytes for {n} frames of {channels} channel(s), got {size}")
        track = cls.__new__(cls)
        if flac is not None:
            track._set_flac(flac, subtype, hip)
        track.sample_rate, track.subtype, track.channels, track.n = int(sample_rate), subtype, int(channels), int(n)
        track.bytes, track.width = data, width
        return track

    @classmethod
    def resampled(cls, audio, sample_rate: int, out_rate: int, n_out: int, subtype: str = "PCM_24", *, hip=None, dev=None,
                  flac: Optional[Dict[str, object]] = None) -> "PackedTrack":
        """This track (at `sample_rate`), resampled to `out_rate` and cropped to `n_out` frames (`output.sample_rate`): with a
        context, one launch of `ac_resample_poly_pack` on the device track (`utils/rate_export.py`) and one download of the
        finished bytes - no float track at `out_rate` exists anywhere; without one, `resample_pack_host`.  `sample_rate` of the
        result is `out_rate`; equal rates give the constructor's bytes, cropped."""
        from .rate_export import rate_ratio, resample_pack_device, resample_pack_host
        subtype_info(subtype)
        up, down = rate_ratio(out_rate, sample_rate)
        channels = _channels_of(np.asarray(audio) if dev is None else dev)
        if hip is not None:
            d = dev if dev is not None else hip.to_device(np.ascontiguousarray(audio, dtype=np.float32))
            data = resample_pack_device(hip, d, up, down, subtype, int(n_out))
            data = data.cpu().numpy() if flac is None else data.contiguous()       # FLAC: the bytes stay on the device
        else:
            data = resample_pack_host(np.asarray(audio), up, down, subtype, int(n_out))
        return cls.from_bytes(data, int(n_out), channels, int(out_rate), subtype, flac=flac, hip=hip)

    @classmethod
    def finished(cls, audio, sample_rate: int, spans, settings, subtype: str = "PCM_24", *, hip=None, dev=None,
                 flac: Optional[Dict[str, object]] = None) -> "PackedTrack":
        """This track with every span of `spans` finished (`utils/segment_finish.py`: a fade at each end, one gain per span from the
        RMS of the faded span) and everything outside the spans as the constructor converts it: still a whole-track buffer, so
        `write(lo, hi)` works as ever.  With a context: the stats launch (when normalising), one launch of `acf_pack_spans` on the
        device track and one download; without one, `finish_host` + `pcm_bytes_host`.  The result carries `finish_rows`, one dict
        per span (`gain`, `gain_db`, `rms_db`, `peak_out`, `clipped`)."""
        from .segment_finish import finished
        return finished(audio, sample_rate, spans, settings, subtype, hip=hip, dev=dev, flac=flac)

    @classmethod
    def from_pcm24(cls, data, n: int, channels: int, sample_rate: int) -> "PackedTrack":
        """`from_bytes` for PCM_24."""
        return cls.from_bytes(data, n, channels, sample_rate, "PCM_24")

    # -- the FLAC form ------------------------------------------------------------------------------------------------------
    def _set_flac(self, flac: Dict[str, object], subtype: str, hip) -> None:
        from .flac_export import checked_options, flac_subtype_width
        self.flac = checked_options(flac)
        flac_subtype_width(subtype)             # PCM_16 or PCM_24: the words FLAC frames are made of here
        self.hip = hip
        self._flac_files: Dict[Tuple[int, int], bytes] = {}

    @property
    def ext(self) -> str:
        """The extension of the files this track writes."""
        return "wav" if self.flac is None else "flac"

    def _clamped(self, start: int, end: Optional[int]) -> Tuple[int, int]:
        end = self.n if end is None else end
        start = max(0, min(int(start), self.n))
        return start, max(start, min(int(end), self.n))

    def prepare(self, spans) -> None:
        """FLAC form: encode every span of `spans` that `write` will be asked for, all in one call (a WAV track does nothing)."""
        if self.flac is None:
            return
        todo = []
        for lo, hi in spans:
            key = self._clamped(lo, hi)
            if key[1] > key[0] and key not in self._flac_files and key not in todo:
                todo.append(key)
        if not todo:
            return
        block, md5 = int(self.flac["block_size"]), bool(self.flac["md5"])
        if isinstance(self.bytes, np.ndarray):
            from .flac_export import flac_encode_host
            files = flac_encode_host(self.bytes, self.n, self.channels, self.width, self.sample_rate, todo, block, md5)
        else:
            from .._flac_native import FlacKernels
            files = FlacKernels(self.hip).encode(self.bytes, self.n, self.channels, self.width, self.sample_rate, todo, block, md5)
        self._flac_files.update(zip(todo, files))

    def _write_flac(self, path: Path, start: int, end: int) -> Path:
        from .flac_export import flac_header
        if end == start:                        # no samples: STREAMINFO alone
            data = flac_header(self.sample_rate, self.channels, 8 * self.width, 0, int(self.flac["block_size"]), 0, 0)
        else:
            self.prepare([(start, end)])
            data = self._flac_files.pop((start, end))
        with open(path, "wb") as fh:
            fh.write(data)
        return Path(path)

    def write(self, path: Path, start: int = 0, end: Optional[int] = None) -> Path:
        if self.flac is not None:
            return self._write_flac(path, *self._clamped(start, end))
        end = self.n if end is None else end
        start = max(0, min(int(start), self.n)); end = max(start, min(int(end), self.n))
        frame = self.width * self.channels
        with open(path, "wb") as fh:
            fh.write(wav_header(end - start, self.sample_rate, self.channels, self.width, self.subtype))
            fh.write(memoryview(self.bytes)[start * frame: end * frame])
            fh.write(wav_pad(end - start, self.channels, self.width))
        return Path(path)


def export_audio(audio: np.ndarray, sample_rate: int, base_path: Path, format_name: str, *, options: Optional[Dict[str, object]] = None) -> Path:
    key = ensure_supported_format(format_name)
    opts = build_export_options(key, options)
    path = _export_path(Path(base_path), key)
    arr = np.asarray(audio)
    _channels_of(arr)
    PackedTrack(arr, sample_rate, str(opts.get("subtype", "PCM_24")), flac=opts if key == "flac" else None).write(path)
    return path


@dataclass
class ExportResult:
    saved_files: List[str] = field(default_factory=list)
    mix_segment_files: List[str] = field(default_factory=list)
    vocal_segment_files: List[str] = field(default_factory=list)
    full_vocal_file: Optional[str] = None
    full_instrumental_file: Optional[str] = None


class SegmentExporter:
    """`segment_exporter.py:25-110`: `segment_{index:03d}_{human|music}[_lib]{suffix}[_{duration:.1f}].{ext}`.

    `export_segments` / `export_full_track` keep the reference's array-in signatures; `export_spans` is the form the
    device path uses (one PackedTrack converted on the GPU, every piece a byte range of it)."""

    def __init__(self, sample_rate: int = 44100) -> None:
        self.sample_rate = sample_rate

    @staticmethod
    def _stem(i: int, n_samples: int, sample_rate: int, *, segment_is_vocal, lib_flags, lib_suffix: str, file_suffix: str,
              duration_map, index_offset: int, always_append_duration: bool) -> str:
        label = "human" if (bool(segment_is_vocal[i]) if i < len(segment_is_vocal) else True) else "music"
        lib = lib_suffix if (lib_flags is not None and i < len(lib_flags) and bool(lib_flags[i])) else ""
        seconds: Optional[float] = None
        if duration_map is not None and i in duration_map:
            seconds = max(0.0, float(duration_map[i]))
        elif always_append_duration:
            seconds = n_samples / float(sample_rate)
        tail = file_suffix if seconds is None else f"{file_suffix}_{seconds:.1f}"
        return f"segment_{i + index_offset:03d}_{label}{lib}{tail}"

    def export_segments(self, segments: Sequence[np.ndarray], output_dir: str, *, segment_is_vocal: Sequence[bool], export_format: str,
                        export_options: Optional[Dict[str, object]], lib_flags: Optional[Sequence[bool]] = None, lib_suffix: str = "_lib",
                        subdir: Optional[str] = None, file_suffix: str = "", duration_map: Optional[Dict[int, float]] = None,
                        index_offset: int = 1, always_append_duration: bool = False) -> List[str]:
        base = Path(output_dir) / subdir if subdir else Path(output_dir)
        base.mkdir(parents=True, exist_ok=True)
        saved: List[str] = []
        for i, piece in enumerate(segments):
            stem = self._stem(i, len(piece), self.sample_rate, segment_is_vocal=segment_is_vocal, lib_flags=lib_flags,
                              lib_suffix=lib_suffix, file_suffix=file_suffix, duration_map=duration_map, index_offset=index_offset,
                              always_append_duration=always_append_duration)
            saved.append(str(export_audio(piece, self.sample_rate, base / stem, export_format, options=export_options)))
        return saved

    def export_spans(self, track: PackedTrack, spans: Sequence[Tuple[int, int]], output_dir: str, *, segment_is_vocal: Sequence[bool],
                     lib_flags: Optional[Sequence[bool]] = None, lib_suffix: str = "_lib", subdir: Optional[str] = None,
                     file_suffix: str = "", duration_map: Optional[Dict[int, float]] = None, index_offset: int = 1,
                     always_append_duration: bool = False) -> List[str]:
        base = Path(output_dir) / subdir if subdir else Path(output_dir)
        base.mkdir(parents=True, exist_ok=True)
        saved: List[str] = []
        track.prepare(spans)                    # the FLAC form encodes all of them in one call
        for i, (lo, hi) in enumerate(spans):
            stem = self._stem(i, hi - lo, track.sample_rate, segment_is_vocal=segment_is_vocal, lib_flags=lib_flags,
                              lib_suffix=lib_suffix, file_suffix=file_suffix, duration_map=duration_map, index_offset=index_offset,
                              always_append_duration=always_append_duration)
            saved.append(str(track.write(_export_path(base / stem, track.ext), lo, hi)))
        return saved

    def export_full_track(self, audio, output_base: Path, *, export_format: str = "wav",
                          export_options: Optional[Dict[str, object]] = None) -> str:
        """`audio`: a PackedTrack (device path) or a mono array (the reference's form)."""
        Path(output_base).parent.mkdir(parents=True, exist_ok=True)
        if isinstance(audio, PackedTrack):
            ensure_supported_format(export_format)
            return str(audio.write(_export_path(Path(output_base), audio.ext)))
        return str(export_audio(audio, self.sample_rate, Path(output_base), export_format, options=export_options))


__all__ = ["ensure_supported_format", "build_export_options", "export_audio", "ExportResult", "SegmentExporter", "PackedTrack",
           "wav_header", "wav_pad", "pcm_bytes_host", "WAV_SUBTYPES", "subtype_info", "configured_subtype", "configured_flac_options"]
