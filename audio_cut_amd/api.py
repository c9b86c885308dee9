"""Public entry point — keeps the reference's `audio_cut.api.separate_and_segment` signature
(`src/audio_cut/api.py:31-45`): load -> (resample) -> separate -> detect -> finalize -> boundary policy -> export ->
SegmentManifest.

`segments` (`few` / `medium` / `many`, `"MIN-MAX"` or `(min_s, max_s)`) and `alignment` (`lyric` / `lyric_lean` / `balanced` /
`beat_lean` / `beat` or 0..1) are the smart-cut intent: given either, the default mode is `vpbd_asr`, the lyrics provider is `auto`,
and the splitter derives planner, scorer, detector and layout settings from them and from the track's estimated style
(AutoProfile, `config/auto_profile.py`); the manifest carries `intent` and `auto_profile` (`smart_cut`).

Modes `v2.2_mdd` (default when no intent arguments are given, `api.py:74-75`), `v2.1`, `vpbd_acoustic`, `vpbd_asr` (the VPBD pool
with a lyrics provider's timeline: `<name>_vocal_for_asr.wav`, the 16 kHz 16-bit copy of the vocal stem the provider is given, and a
`lyrics` object per manifest segment), `librosa_onset`
(bar-aligned smart segmentation: mix segments by default, vocal segments on request, no full stems) and
`hybrid_mdd` (phrase-pause cuts snapped to beats in chorus bars: mix and vocal segments named `..._lib_D.D` where a segment ends on
a beat, and the full vocal) and `vocal_separation` (the two stems and nothing else: `<name>_vocal_D.D.wav` and
`<name>_instrumental_D.D.wav`, no detection, no segments).
Loader: WAV / .npy.  WAVs are read by `utils/wav_reader.py`: PCM of 8, 16, 24 and 32 bits and IEEE float of 32 and 64, plain or
WAVE_FORMAT_EXTENSIBLE, 1 to 8 channels; companded and compressed files, RF64 and RIFX are refused by name ("Input
files").  With `audio.gpu_decode` (default true) a `.wav` is decoded on the device (`load_audio_device`): the file's own bytes are
read into pinned memory and uploaded, and one kernel (`ac_decode_pcm`) leaves the float32 track resident - bit for bit what
`load_audio_mono` / `load_audio_stereo` decode on the host, which `.npy` input and `audio.gpu_decode: false` still go through.  The
channel mean is `librosa.load(mono=True)`'s; a float file holding a NaN or an infinity is refused.  A file whose rate differs from
`audio.sample_rate` is resampled on the GPU with `ac_resample_poly` (= scipy.signal.resample_poly; the reference's soxr_hq is not
available offline, so this row's parity definition is the scipy filter — SURVEY.md §8(f) row 2).
Export (`seamless_splitter.py:674-731`): `segment_NNN_{human|music}_D.D.wav` mix segments, `segments_vocal/..._vocal_D.D.wav`,
`<name>_<mode>_vocal_full_D.D.wav`, `<name>_<mode>_instrumental_D.D.wav`, all of the subtype `output.wav.subtype` names (default PCM_24), packed on the GPU (`ac_pack_pcm`).
With `output.format: flac` the same files are `.flac`: the packed bytes stay on the device and are encoded there (`utils/flac_export.py`,
`_flac_native.py`), decoding to exactly the samples of the WAV of that subtype; the result then carries `export_format`.
`output.sample_rate` (`"source"` or an integer; absent by default; INTEGRATION.md, "Export rate") lets the files leave at another rate than
`audio.sample_rate`: the stems through `ac_resample_poly_pack` (`utils/rate_export.py`), the mix at the file's own rate as it was loaded.
Manifest: `_build_manifest` (`api.py:178-263`) key for key, QA report included, and the lyrics attachment to segments where an alignment
ran.  `separate_and_segment` returns the manifest like the reference's does.

`audio.channels` (1 or 2, validated like `config_manager.py:353-354`): with 2 the file is loaded as planar (2, N) float32
(`load_audio_stereo`; a mono file goes to both channels), the network separates true L/R, and every exported WAV has two
channels.  Detection runs on the channel mean.  A file at another rate is resampled per channel first and detection sees the
mean of the resampled channels, whereas `channels: 1` takes the mean first and resamples the mono track; the two orders
round differently, so the same file may give different cut samples with 1 and 2 channels.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, Mapping, Optional, Sequence

import numpy as np

from . import config as _config
from .config.auto_profile import resolve_smart_cut_intent
from .core.seamless_splitter import SeamlessSplitter
from .lyrics.models import LyricsTimeline
from .lyrics.segment_attach import attach_lyrics_to_segments
from .utils.rate_export import map_cut, rate_ratio, resampled_len, resolve_output_rate
from .utils.wav_reader import LAYOUT_MONO, LAYOUT_PLANAR, channel_mean, read_wav, read_wav_bytes, read_wav_info


def _read_wav(p: Path) -> tuple:
    """PCM 8/16/24/32 or float 32/64 WAV, plain or WAVE_FORMAT_EXTENSIBLE -> (float32 [frames, channels], sample_rate).  PCM lies in
    [-1, 1); float samples pass as they are."""
    return read_wav(p)


def load_audio_mono(path: str) -> tuple:
    """WAV (`utils/wav_reader.py`) or .npy -> (mono float32, sample_rate).  Channel mean like `librosa.load(mono=True)`: the float32
    sum in channel order over float32(channels), which is `np.mean(axis=1)` bit for bit for up to six channels."""
    p = Path(path)
    if p.suffix.lower() == ".npy":
        arr = np.load(p)
        return (np.mean(arr, axis=0) if arr.ndim == 2 else arr).astype(np.float32), 44100
    data, sr = _read_wav(p)
    return channel_mean(data), sr


def load_audio_stereo(path: str) -> tuple:
    """WAV or .npy -> (planar float32 (2, N), sample_rate) for `audio.channels: 2`.  A mono file (a 1-D
    or (1, N) array, a 1-channel WAV) is duplicated to both channels; more than two channels is refused.  `.npy` arrays are
    (channels, N) like the mono loader reads them, at 44100 Hz."""
    p = Path(path)
    if p.suffix.lower() == ".npy":
        arr, sr = np.asarray(np.load(p), dtype=np.float32), 44100
        arr = arr[None, :] if arr.ndim == 1 else arr
        if arr.ndim != 2:
            raise ValueError(f"{p}: expected a 1-D or (channels, N) array, got shape {arr.shape}")
    else:
        data, sr = _read_wav(p)
        arr = data.T
    if arr.shape[0] == 1:
        arr = np.concatenate([arr, arr], axis=0)
    if arr.shape[0] != 2:
        raise ValueError(f"{p}: {arr.shape[0]} channels; audio.channels: 2 takes mono or stereo input")
    return np.ascontiguousarray(arr, dtype=np.float32), sr


def load_audio_device(path: str, hip, channels: int = 1) -> tuple:
    """WAV -> (the track resident on `hip`'s device, sample_rate) without decoding on the host: the header walk
    (`read_wav_info`), one read of the sample bytes straight into pinned memory, one asynchronous copy on the current stream and
    one `ac_decode_pcm`.  `channels=1`: float32 [N], the channel mean (`load_audio_mono`'s bits); `channels=2`: planar float32
    [2, N] (`load_audio_stereo`'s: a mono file goes to both channels, more than two are refused).  A float file with a NaN or an
    infinity in it is refused with the count, as `librosa.load` refuses it (`valid_audio`).  Pinned staging was measured against
    pageable memory (the loader) and is 3 to 4 times faster for a stereo track."""
    import torch
    p = Path(path)
    channels = _check_channels(channels)
    info = read_wav_info(p)
    if channels == 2 and info.channels > 2:
        raise ValueError(f"{p}: {info.channels} channels; audio.channels: 2 takes mono or stereo input")
    staged = torch.empty(info.data_bytes, dtype=torch.uint8, pin_memory=True)
    read_wav_bytes(p, info, into=staged.numpy())
    with torch.cuda.device(hip.device):
        raw_dev = staged.to(hip.device, non_blocking=True)      # the caching host allocator keeps the block until the copy has run
        if channels == 1:
            track, bad = hip.decode_pcm(raw_dev, info, LAYOUT_MONO)
        elif info.channels == 2:
            track, bad = hip.decode_pcm(raw_dev, info, LAYOUT_PLANAR)
        else:
            track = torch.empty((2, info.n_frames), dtype=torch.float32, device=hip.device)
            _, bad = hip.decode_pcm(raw_dev, info, LAYOUT_MONO, out=track[0])
            track[1].copy_(track[0])
    if bad:
        raise ValueError(f"{p}: {bad} samples are NaN or infinite")
    return track, info.sample_rate


def _check_channels(value: Any) -> int:
    """`config_manager.py:353-354`: audio.channels must be 1 or 2."""
    if value not in (1, 2):
        raise ValueError(f"unsupported audio.channels: {value!r} (1 or 2)")
    return int(value)


def _sha256(path: Path) -> str:
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def _rel(path: str, root: Path) -> str:
    try:
        return Path(path).resolve().relative_to(Path(root).resolve()).as_posix()
    except Exception:
        return Path(path).as_posix()


def _normalize_export_plan(export_types: Optional[Sequence[str]]) -> list:
    """`_normalize_export_plan` (`seamless_splitter.py:107-153`): the four artifact kinds, default all."""
    allowed = ("mix_segments", "vocal_segments", "full_vocal", "full_instrumental")
    if not export_types:
        return list(allowed)
    plan = []
    for item in export_types:
        key = str(item).strip().lower()
        if key in ("all", "*"):
            return list(allowed)
        if key not in allowed:
            raise ValueError(f"unknown export type {item!r}; choose from {allowed}")
        if key not in plan:
            plan.append(key)
    return plan


def _vocal_separation_plan(export_types: Optional[Sequence[str]]) -> set:
    """Mode `vocal_separation`: `_normalize_export_plan(export_plan, default=('full_vocal', 'full_instrumental'))`
    (`seamless_splitter.py:107-153,975-978`).  No plan, an empty one or one of blanks is the default; `all` adds the default, `none`
    empties the plan; the reference's aliases are taken; a segment kind stays in the plan and writes nothing (`:984,996`).  A token
    that names no kind is refused as in the other modes."""
    default = ("full_vocal", "full_instrumental")
    alias = {"vocal": "full_vocal", "vocal_full": "full_vocal", "instrumental": "full_instrumental",
             "instrumental_full": "full_instrumental", "human_segments": "vocal_segments", "human": "vocal_segments",
             "music_segments": "mix_segments", "music": "mix_segments"}
    allowed = ("mix_segments", "vocal_segments", "full_vocal", "full_instrumental")
    if export_types is None:
        return set(default)
    flags: set = set()
    for item in export_types:
        key = "" if item is None else str(item).strip().lower()
        if not key:
            continue
        if key == "none":
            return set()
        if key == "all":
            flags.update(default)
            continue
        key = alias.get(key, key)
        if key not in allowed:
            raise ValueError(f"unknown export type {item!r}; choose from {allowed}")
        flags.add(key)
    return flags or set(default)


def _export_vocal_separation(res: Mapping[str, Any], in_path: Path, out_dir: Path, export_types: Optional[Sequence[str]], sr: int,
                             t_start: float) -> Dict[str, Any]:
    """The export half of `_process_vocal_separation_only` (`seamless_splitter.py:975-1036`): `<name>_vocal_<seconds:.1f>.wav` and
    `<name>_instrumental_<seconds:.1f>.wav` from the sample bytes the separation produced, and the reference's result dict.  The
    bytes are of the subtype `separate_only` read from `output.wav.subtype` and recorded next to them (absent: PCM_24)."""
    import time
    from .utils.audio_export import PackedTrack, SegmentExporter
    plan = _vocal_separation_plan(export_types)
    pcm = res["stem_pcm24"]
    subtype = pcm.get("subtype", "PCM_24")
    flac = pcm.get("flac")                  # `output.format: flac`: the stems are device tensors, encoded there
    seconds = int(pcm["n"]) / float(sr)
    exporter = SegmentExporter(sr)
    files: Dict[str, Optional[str]] = {"vocal": None, "instrumental": None}
    saved = []
    for kind in ("vocal", "instrumental"):
        if f"full_{kind}" in plan and pcm.get(kind) is not None:      # no instrumental: the reference logs it and goes on (`:1007-1008`)
            track = PackedTrack.from_bytes(pcm[kind], int(pcm["n"]), int(pcm["channels"]), sr, subtype, flac=flac, hip=pcm.get("hip"))
            files[kind] = exporter.export_full_track(track, out_dir / f"{in_path.stem}_{kind}_{seconds:.1f}")
            saved.append(files[kind])
    out: Dict[str, Any] = {
        "success": True, "mode": "vocal_separation", "method": res["method"], "num_segments": 0, "saved_files": saved,
        "mix_segment_files": [], "vocal_segment_files": [], "full_vocal_file": files["vocal"],
        "full_instrumental_file": files["instrumental"], "export_plan": sorted(plan), "backend_used": res.get("backend_used"),
        "separation_confidence": res.get("separation_confidence"), "processing_time": time.time() - t_start,
        "segment_durations": [], "guard_shift_stats": dict(res["guard_shift_stats"]),
        "precision_guard_ok": bool(res["precision_guard_ok"]), "precision_guard_threshold_ms": dict(res["precision_guard_threshold_ms"]),
        "input_file": str(in_path), "output_dir": str(out_dir), "sample_rate": sr, "timings": res.get("timings", {}),
    }
    if flac is not None:
        out["export_format"] = "flac"
    out.update(res.get("gpu_meta", {}))
    return out


def separate_and_segment(*, input_uri: str, export_dir: str, mode: Optional[str] = None, segments: Optional[Any] = None,
                         alignment: Optional[Any] = None, device: Optional[str] = None,
                         export_types: Optional[Sequence[str]] = None, layout: Optional[Any] = None,
                         strict_gpu: Optional[bool] = None, export_manifest: bool = False,
                         manifest_filename: str = "SegmentManifest.json",
                         runtime_overrides: Optional[Dict[str, Any]] = None) -> Dict:
    """Returns the SegmentManifest dict (`api.py:115-131`); with `export_manifest` it is also written under `export_dir`
    and carries `manifest_path`.  The splitter's own result (`split_audio_seamlessly`'s dict) is `last_result()`."""
    has_intent = segments is not None or alignment is not None
    in_path = Path(input_uri).expanduser().resolve()
    if not in_path.exists():
        raise FileNotFoundError(f"input audio not found: {in_path}")
    out_dir = Path(export_dir).expanduser().resolve()
    out_dir.mkdir(parents=True, exist_ok=True)
    resolved_mode = mode or ("vpbd_asr" if has_intent else "v2.2_mdd")     # `api.py:74-75`: an explicit mode wins
    saved = _config.snapshot()
    try:
        overrides: Dict[str, Any] = {}
        if device:
            overrides["gpu_pipeline.prefer_device"] = device          # api.py:155-156
        if strict_gpu is not None:
            overrides["gpu_pipeline.strict_gpu"] = bool(strict_gpu)
        if layout:                                                       # api.py:161-166
            lay = dict(layout)
            overrides["segment_layout.enable"] = bool(lay.pop("enable", True))
            for k, v in lay.items():
                overrides[f"segment_layout.{k}"] = v
        if has_intent:                                                   # `_build_intent_runtime_overrides` (`api.py:134-144`)
            overrides.update({"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "auto", "lyrics_alignment.strict": False})
            if segments is not None:
                overrides["smart_cut.segments"] = segments
            if alignment is not None:
                overrides["smart_cut.alignment"] = alignment
        overrides.update(dict(runtime_overrides or {}))                 # explicit dotted overrides are applied last (`:168-175`)
        # written like the reference writes them, straight into the tree (`:147-175`): they override, and the smart-cut layer does
        # not read them as keys the caller set on purpose (`config.get_runtime_override_keys`)
        _config.set_runtime_config(overrides, explicit=False)
        intent_echo = resolve_smart_cut_intent(_config.get_config("smart_cut", {}) or {}) if has_intent else None   # `:97-100`
        layout_cfg = dict(_config.get_config("segment_layout", {}) or {})
        sr = int(_config.get_config("audio.sample_rate", 44100))
        channels = _check_channels(_config.get_config("audio.channels", 1))
        result = _split_and_export(in_path, out_dir, resolved_mode, export_types, sr, device, channels)
        if intent_echo is not None:
            result.setdefault("intent", intent_echo)                    # the splitter's own record, with `applied_overrides`, stays
    finally:
        _config.restore(saved)
    global _LAST_RESULT
    _LAST_RESULT = result
    manifest = _build_manifest(result=result, input_path=in_path, export_dir=out_dir, mode=resolved_mode, sample_rate=sr,
                               channels=channels, layout_cfg=layout_cfg)
    if export_manifest:
        path = out_dir / manifest_filename
        path.write_text(json.dumps(manifest, ensure_ascii=False, indent=2, default=str), encoding="utf-8")
        manifest["manifest_path"] = path.as_posix()
    return manifest


_LAST_RESULT: Optional[Dict[str, Any]] = None


def last_result() -> Optional[Dict[str, Any]]:
    """The result dict behind the most recent manifest of this process (cut samples, file lists, per-phase timings)."""
    return _LAST_RESULT


# the segment-finishing keys of `quality_control` and their defaults (config/__init__.py): with all five there, nothing of the feature
# is imported and the finish library is not opened
_FINISH_DEFAULTS = {"fade_in_duration": 0.0, "fade_out_duration": 0.0, "normalize_audio": False, "normalize_target_db": -20.0,
                    "normalize_max_gain": 10.0}


def _configured_finish(sr: int):
    """The `FinishSettings` of an export whose segments are to be faded or normalised, else None.  A key off its default is read -
    and refused by name if it cannot be honoured - before any work."""
    if all(_config.get_config(f"quality_control.{k}", d) in (d, None) for k, d in _FINISH_DEFAULTS.items()):
        return None
    from .utils.segment_finish import configured_finish
    settings = configured_finish(sr)
    return settings if settings.active else None


def _finish_keys_in_force(finish) -> list:
    return [f"quality_control.{k}" for k, on in (("fade_in_duration", finish.fade_in_frames > 0),
                                                 ("fade_out_duration", finish.fade_out_frames > 0),
                                                 ("normalize_audio", finish.normalize_audio)) if on]


def _split_and_export(in_path: Path, out_dir: Path, mode: str, export_types: Optional[Sequence[str]], sr: int,
                      device: Optional[str], channels: int = 1) -> Dict[str, Any]:
    """The reference's `split_audio_seamlessly` for the modes built here (`seamless_splitter.py:171-253,270-760`): load,
    split, export, and the result dict `_build_manifest` reads.  `channels == 2`: the planar stereo track is split (true-stereo
    separation, detection on its channel mean) and every file is written with both channels."""
    import time
    from .utils.audio_export import ExportResult, PackedTrack, SegmentExporter, configured_flac_options, configured_subtype
    t_start = time.time()
    subtype = configured_subtype()          # `output.format` / `output.wav.subtype`: refused here, before any work, if not written
    # `output.format: flac` (utils/flac_export.py): the checked `output.flac` settings, else None - and then every call below is
    # the call of a build without the format
    flac = configured_flac_options()
    fkw = {} if flac is None else {"flac": flac}
    finish = _configured_finish(sr)         # segment finishing (utils/segment_finish.py); None with the keys at their defaults
    # `output.sample_rate` (utils/rate_export.py): the rate the files leave at, resolved - and refused - from the file's header
    # alone, before the track is loaded.  Absent: `out_sr` is `sr` and nothing below differs from a build without the setting.
    rate_set = _config.get_config("output.sample_rate", None) is not None
    out_sr, source_sr = sr, sr
    if rate_set:
        source_sr = sr if in_path.suffix.lower() == ".npy" else int(read_wav_info(in_path).sample_rate)
        out_sr = resolve_output_rate(source_sr, sr)
        if mode == "vocal_separation" and out_sr != sr:
            raise ValueError(f"output.sample_rate {out_sr} with mode 'vocal_separation': that mode writes its bytes straight from the "
                             f"iSTFT and has no float stem to resample, so it exports at audio.sample_rate ({sr}) only; mode "
                             f"'v2.2_mdd' with export_types=[\"full_vocal\", \"full_instrumental\"] writes the same two files at {out_sr} Hz")
        if finish is not None and out_sr != sr:
            raise ValueError(f"{', '.join(_finish_keys_in_force(finish))} with output.sample_rate {out_sr}: segments are finished at "
                             f"audio.sample_rate ({sr}) only, the resampling export does not know where the segments are; leave "
                             f"output.sample_rate unset (or at {sr}), or the finishing keys at their defaults")
    splitter = SeamlessSplitter(sample_rate=sr, device=device)
    hip = splitter._context()
    audio_dev = None
    source_track = None         # the track in front of the load resampler (device or host), kept when the files leave at its rate
    if in_path.suffix.lower() == ".wav" and bool(_config.get_config("audio.gpu_decode", True)):
        # the file's bytes are decoded on the device (`load_audio_device`); the host copy of the track is one download
        audio_dev, file_sr = load_audio_device(str(in_path), hip, channels)
        if file_sr != sr:                     # as below: per channel for two channels, the mono mean for one
            import torch
            source_track = audio_dev if out_sr == file_sr else None
            audio_dev = torch.stack([hip.resample_poly(audio_dev[c].contiguous(), sr, file_sr) for c in range(2)]) if channels == 2 \
                else hip.resample_poly(audio_dev, sr, file_sr)
        audio = audio_dev.cpu().numpy()
    elif channels == 2:
        audio, file_sr = load_audio_stereo(str(in_path))
        if file_sr != sr:                     # each channel on its own; detection then reads the mean of the resampled channels
            import torch
            source_track = audio if out_sr == file_sr else None
            audio_dev = torch.stack([hip.resample_poly(hip.to_device(audio[c]), sr, file_sr) for c in range(2)])
            audio = audio_dev.cpu().numpy()
    else:
        audio, file_sr = load_audio_mono(str(in_path))
        if file_sr != sr:
            source_track = audio if out_sr == file_sr else None
            audio_dev = hip.resample_poly(hip.to_device(audio), sr, file_sr)     # e.g. 48 kHz -> 44.1 kHz = up 147 / down 160
            audio = audio_dev.cpu().numpy()
    # `vpbd_asr`: the detector writes the 16 kHz ASR copy of the vocal stem next to the exports, named after the input
    res = splitter.split_track(audio, mode=mode, audio_dev=audio_dev, input_path=str(in_path), output_dir=str(out_dir))
    if not res.get("success", True):                    # `split_audio_seamlessly`'s failure result (`:231-233`): nothing is written
        return {"success": False, "error": res.get("error"), "input_file": str(in_path), "mode": mode,
                "timings": res.get("timings", {}), "processing_time": time.time() - t_start}
    if mode == "vocal_separation":
        return _export_vocal_separation(res, in_path, out_dir, export_types, sr, t_start)
    smart = mode == "librosa_onset"
    hybrid = mode == "hybrid_mdd"
    single = bool(res.get("single_segment"))            # `_create_single_segment_result`: only the mix, no duration tag
    if smart:       # `:1291-1322`: the mix segments by default; of the other kinds only the vocal segments are written in this mode
        plan = [k for k in _normalize_export_plan(export_types) if k in ("mix_segments", "vocal_segments")] if export_types \
            else ["mix_segments"]
    elif hybrid:    # `:1580-1629`: mix and vocal segments and the full vocal; this mode writes no instrumental
        kinds = ("mix_segments", "vocal_segments", "full_vocal")
        plan = [k for k in _normalize_export_plan(export_types) if k in kinds] if export_types else list(kinds)
    else:
        plan = _normalize_export_plan(export_types) if (export_types or not single) else ["mix_segments"]
    cuts = [int(c) for c in res.get("cuts_samples", res["sample_boundaries"])]
    spans = [tuple(sp) for sp in res.get("segment_spans", list(zip(cuts[:-1], cuts[1:])))]
    flags = list(res.get("segment_vocal_flags", [True] * len(spans)))
    durations = [(hi - lo) / float(sr) for lo, hi in spans]
    dmap = None if single else {i: d for i, d in enumerate(durations)}
    # `hybrid_mdd` names its segments `segment_NNN_{human|music}[_lib]_D.D` (`:1586-1616`)
    naming = {"lib_flags": list(res.get("segment_lib_flags", [])), "lib_suffix": res.get("lib_suffix", "_lib"), "index_offset": 1,
              "always_append_duration": True} if hybrid else {}
    exp = ExportResult()
    exporter = SegmentExporter(sr)
    state = res.get("device_state") or {}
    # the tracks written: mono, or with two channels the stereo mix and stems ([2, N], host and device)
    st = "_stereo" if channels == 2 else ""
    mix_dev = state.get("mix_stereo", audio_dev) if channels == 2 else state.get("mix", audio_dev)
    n = int(np.shape(audio)[-1])
    if out_sr == sr:
        n_out, out_spans = n, spans

        def packed(track, dev):
            return PackedTrack(track, sr, subtype, hip=hip, dev=dev, **fkw)
    else:
        # every exported track has n_out frames: the file's own count at the file's rate (the stems are cropped to it, never padded),
        # else what the resampler gives; every span end goes to its nearest frame there and the end of the track to n_out, so the
        # segments of a kind are consecutive byte ranges of the one converted track
        n_out = int(np.shape(source_track)[-1]) if source_track is not None else resampled_len(n, *rate_ratio(out_sr, sr))
        out_spans = [(map_cut(lo, sr, out_sr, n_out, n), map_cut(hi, sr, out_sr, n_out, n)) for lo, hi in spans]

        def packed(track, dev):
            return PackedTrack.resampled(track, sr, out_sr, n_out, subtype, hip=hip, dev=dev, **fkw)
    if "mix_segments" in plan:
        if finish is not None:              # out_sr == sr here: the spans are finished where the track becomes bytes
            mix_pk = PackedTrack.finished(audio, sr, spans, finish, subtype, hip=hip, dev=mix_dev, **fkw)
        elif source_track is not None:      # the loaded track as it was in front of the load resampler: nothing is resampled twice
            is_dev = not isinstance(source_track, np.ndarray)
            mix_pk = PackedTrack(source_track, out_sr, subtype, hip=hip, dev=source_track if is_dev else None, **fkw)
        else:
            mix_pk = packed(audio, mix_dev)
        exp.mix_segment_files = exporter.export_spans(mix_pk, out_spans, str(out_dir), segment_is_vocal=flags, duration_map=dmap,
                                                      **naming)
        exp.saved_files += exp.mix_segment_files
    vocal = res.get("vocal_track" + st)
    # finishing: the full vocal stays plain, so the segments come from a second, finished conversion of the stem
    plain_vocal = "full_vocal" in plan or ("vocal_segments" in plan and finish is None)
    voc_pk = packed(vocal, state.get("vocal" + st)) if (vocal is not None and plain_vocal) else None
    voc_seg_pk = voc_pk if finish is None else (
        PackedTrack.finished(vocal, sr, spans, finish, subtype, hip=hip, dev=state.get("vocal" + st), **fkw)
        if (vocal is not None and "vocal_segments" in plan) else None)
    if flac is not None and voc_pk is not None and voc_seg_pk is voc_pk and "vocal_segments" in plan and "full_vocal" in plan:
        voc_pk.prepare(list(out_spans) + [(0, voc_pk.n)])      # the segments and the full stem in one encoder call
    if "vocal_segments" in plan and voc_seg_pk is not None:
        exp.vocal_segment_files = exporter.export_spans(voc_seg_pk, out_spans, str(out_dir), segment_is_vocal=flags, subdir="segments_vocal",
                                                        file_suffix="_vocal", duration_map=dmap, **naming)
        exp.saved_files += exp.vocal_segment_files
    if "full_vocal" in plan and voc_pk is not None:
        exp.full_vocal_file = exporter.export_full_track(voc_pk, out_dir / f"{in_path.stem}_{mode}_vocal_full_{np.shape(vocal)[-1] / float(sr):.1f}")
        exp.saved_files.append(exp.full_vocal_file)
    inst = res.get("instrumental_track" + st)
    if "full_instrumental" in plan and inst is not None:
        inst_pk = packed(inst, state.get("instrumental" + st))
        exp.full_instrumental_file = exporter.export_full_track(inst_pk, out_dir / f"{in_path.stem}_{mode}_instrumental_{np.shape(inst)[-1] / float(sr):.1f}")
        exp.saved_files.append(exp.full_instrumental_file)
    out: Dict[str, Any] = {
        "success": True, "mode": mode, "method": res.get("method", f"pure_vocal_split_{mode}"), "input_file": str(in_path), "output_dir": str(out_dir),
        "sample_rate": sr, "guard_boundaries_samples": [int(b) for b in res["sample_boundaries"]],
        "cut_points_samples": cuts, "cut_points_sec": [c / float(sr) for c in cuts],
        "num_segments": len(spans), "segment_durations": durations, "segment_vocal_flags": flags,
        "segment_labels": ["human" if f else "music" for f in flags],
        "segment_classification_debug": list(res.get("segment_classification_debug", [])),
        "segment_layout_applied": bool(res.get("segment_layout_applied", False)),
        "suppressed_cut_points_sec": list(res.get("suppressed_cut_points_sec", [])),
        "guard_adjustments": [dict(getattr(a, "__dict__", a)) for a in res.get("guard_adjustments", [])],
        "guard_shift_stats": dict(res.get("guard_shift_stats", SeamlessSplitter._guard_shift_stats([]))),
        "precision_guard_ok": bool(res.get("precision_guard_ok", True)),
        "precision_guard_threshold_ms": dict(res.get("precision_guard_threshold_ms", {})),
        "separation_confidence": res.get("separation_confidence"), "backend_used": res.get("backend_used"),
        "export_plan": sorted(plan), "saved_files": list(exp.saved_files), "mix_segment_files": list(exp.mix_segment_files),
        "vocal_segment_files": list(exp.vocal_segment_files), "full_vocal_file": exp.full_vocal_file,
        "full_instrumental_file": exp.full_instrumental_file,
        "timings": res.get("timings", {}), "processing_time": time.time() - t_start,
    }
    if flac is not None:        # only when the files are not WAV
        out["export_format"] = "flac"
    if rate_set:        # `output.sample_rate`: what the files are at; `sample_rate` and `cut_points_samples` stay the pipeline's
        out.update({"export_sample_rate": out_sr, "source_sample_rate": source_sr,
                    "export_cut_points_samples": [c if out_sr == sr else map_cut(c, sr, out_sr, n_out, n) for c in cuts]})
    if finish is not None:      # what was measured and applied, segment by segment
        out["segment_finish"] = {
            "settings": finish.as_dict(), "fade_in_frames": finish.fade_in_frames, "fade_out_frames": finish.fade_out_frames,
            "mix": list(getattr(mix_pk, "finish_rows", [])) if "mix_segments" in plan else [],
            "vocal": list(getattr(voc_seg_pk, "finish_rows", [])) if ("vocal_segments" in plan and voc_seg_pk is not None) else []}
    if res.get("note"):
        out["note"] = res["note"]
    if smart:       # `:1341-1347`, and the bar analysis behind the cuts
        for key in ("use_vocal_preprocessing", "bpm", "bar_duration_s", "density", "silence_boundaries", "bar_energies", "bar_types"):
            out[key] = res.get(key)
    if hybrid:      # `result_builder.add_hybrid_metadata` (`result_builder.py:100-116`), and what the strategy counted
        for key in ("segment_lib_flags", "lib_segment_count", "hybrid_config", "beat_analysis", "strategy", "strategy_metadata"):
            out[key] = res.get(key)
    if res.get("boundary_detection") is not None:
        out["boundary_detection"] = res["boundary_detection"]
        out["lyrics_alignment"] = res.get("lyrics_alignment")
        if "lyrics_cut_protection_applied" in res:
            out["lyrics_cut_protection_applied"] = bool(res["lyrics_cut_protection_applied"])
    for key in ("auto_profile", "intent"):              # a smart-cut run (`seamless_splitter.py:761-765`)
        if res.get(key) is not None:
            out[key] = res[key]
    out.update(res.get("gpu_meta", {}))
    return out


def _to_ms(seconds: Any) -> Optional[int]:
    try:
        return None if seconds is None else int(round(float(seconds) * 1000.0))
    except (TypeError, ValueError):
        return None


def _annotated_cuts(result: Mapping[str, Any]) -> list:
    """`_build_final_cuts` (`api.py:307-372`): with a VPBD planner in the result, every cut that is a selected candidate
    (followed through `final_time_by_raw_time`) becomes `{t, score, source, features, reasons, meta[, guard_shift_ms]}`;
    otherwise `cuts.final` is the plain list of seconds."""
    times = list(result.get("cut_points_sec", []))
    vpbd = result.get("boundary_detection")
    if not isinstance(vpbd, Mapping):
        return times
    key = lambda v: round(float(v), 6)
    planner = vpbd.get("planner") if isinstance(vpbd.get("planner"), Mapping) else {}

    def keyed(table: Any) -> Dict[float, Any]:
        out: Dict[float, Any] = {}
        for k, v in (table.items() if isinstance(table, Mapping) else ()):
            try:
                out[key(k)] = v
            except (TypeError, ValueError):
                continue
        return out

    moved: Dict[float, float] = {}
    for raw, t in keyed(planner.get("final_time_by_raw_time")).items():
        try:
            moved[raw] = float(t)
        except (TypeError, ValueError):
            continue
    landed = lambda raw: key(moved.get(raw, raw))
    chosen: Dict[float, Mapping[str, Any]] = {}
    for cand in vpbd.get("selected", []) or []:
        if isinstance(cand, Mapping):
            try:
                chosen[landed(key(cand.get("t")))] = cand
            except (TypeError, ValueError):
                continue
    shifts = {landed(raw): ms for raw, ms in keyed(planner.get("guard_shift_ms_by_raw_time")).items()}
    if not chosen and not shifts:
        return times
    final: list = []
    for t in times:
        try:
            k, entry = key(t), {"t": float(t)}
        except (TypeError, ValueError):
            final.append(t)
            continue
        cand = chosen.get(k)
        if cand is not None:
            entry.update({"score": cand.get("score"), "source": cand.get("source"), "features": dict(cand.get("features") or {}),
                          "reasons": list(cand.get("reasons") or []), "meta": dict(cand.get("meta") or {})})
        if k in shifts:
            entry["guard_shift_ms"] = shifts[k]
        final.append(entry)
    return final


def _manifest_segments(result: Mapping[str, Any], export_dir: Path) -> list:
    """`_build_segments` (`api.py:266-304`).  A result whose lyrics alignment ran (`lyrics_alignment.enabled`: mode `vpbd_asr`
    with a provider switched on, fallbacks included) gets every segment's `lyrics` object - or None - from the timeline
    (`lyrics/segment_attach.py`); every other result keeps its rows as they are."""
    times = list(result.get("cut_points_sec", []))
    durations = list(result.get("segment_durations", []))
    mix, voc = list(result.get("mix_segment_files", [])), list(result.get("vocal_segment_files", []))
    debug = list(result.get("segment_classification_debug", []))
    rows = []
    for i, label in enumerate(result.get("segment_labels", [])):
        start = times[i] if i < len(times) else sum(durations[:i])
        end = times[i + 1] if i + 1 < len(times) else start + (durations[i] if i < len(durations) else 0.0)
        row: Dict[str, Any] = {"id": f"{i + 1:04d}", "start": start, "end": end,
                               "duration": durations[i] if i < len(durations) else end - start, "label": label}
        if i < len(mix):
            row["mix_path"] = _rel(mix[i], export_dir)
        if i < len(voc):
            row["vocal_path"] = _rel(voc[i], export_dir)
        if i < len(debug) and debug[i]:
            row["debug"] = debug[i]
        rows.append(row)
    timeline = _timeline_from_result(result)
    return rows if timeline is None else attach_lyrics_to_segments(rows, timeline)


def _timeline_from_result(result: Mapping[str, Any]):
    """`_timeline_from_result` (`api.py:372-382`): the timeline the result carries, read leniently; None when no alignment ran."""
    block = result.get("lyrics_alignment")
    if not isinstance(block, Mapping) or not block.get("enabled") or not isinstance(block.get("timeline"), Mapping):
        return None
    try:
        return LyricsTimeline.from_dict(dict(block["timeline"]), strict=False)
    except Exception:
        return None


def _track_seconds(result: Mapping[str, Any], input_path: Path) -> Optional[float]:
    """`_estimate_duration` (`api.py:405-431`): the last cut, else the file header, else the summed segment durations."""
    times = result.get("cut_points_sec")
    if times:
        try:
            return float(times[-1])
        except (TypeError, ValueError):
            pass
    try:
        info = read_wav_info(input_path)
        return info.n_frames / float(info.sample_rate)
    except Exception:
        pass
    durations = result.get("segment_durations")
    return float(sum(durations)) if durations else None


def _build_manifest(*, result: Mapping[str, Any], input_path: Path, export_dir: Path, mode: str, sample_rate: int, channels: int,
                    layout_cfg: Mapping[str, Any]) -> Dict[str, Any]:
    """`_build_manifest` (`api.py:178-263`): same keys, same optional blocks, QA report included."""
    from .qa_report import build_qa_report
    input_path, export_dir = Path(input_path), Path(export_dir)
    artifacts: Dict[str, Any] = {}
    for name, field in (("music_segments", "mix_segment_files"), ("human_segments", "vocal_segment_files")):
        if result.get(field):
            artifacts[name] = [_rel(p, export_dir) for p in result[field]]
    for name, field in (("vocal_full", "full_vocal_file"), ("instrumental_full", "full_instrumental_file")):
        if result.get(field):
            artifacts[name] = _rel(result[field], export_dir)
    if result.get("saved_files"):
        artifacts["all"] = [_rel(p, export_dir) for p in result["saved_files"]]
    artifacts["output_dir"] = export_dir.as_posix()
    manifest: Dict[str, Any] = {
        "version": str(mode), "success": bool(result.get("success", False)), "job": {"source": input_path.as_posix()},
        "export_plan": result.get("export_plan") or [],
        "audio": {"sr": sample_rate, "channels": channels, "duration": _track_seconds(result, input_path),
                  "hash": f"sha256:{_sha256(input_path)}"},
        "layout_cfg": dict(layout_cfg) | {"applied": bool(result.get("segment_layout_applied", False))},
        "cuts": {"final": _annotated_cuts(result), "samples": result.get("cut_points_samples", []),
                 "suppressed": result.get("suppressed_cut_points_sec", [])},
        "segments": _manifest_segments(result, export_dir), "artifacts": artifacts,
        "guard": {"shift_stats": result.get("guard_shift_stats", {}), "adjustments": result.get("guard_adjustments", []),
                  "precision_ok": bool(result.get("precision_guard_ok", True)), "threshold_ms": result.get("precision_guard_threshold_ms", {})},
        "separation": {"backend": result.get("backend_used"), "confidence": result.get("separation_confidence")},
        "timings_ms": {"total": _to_ms(result.get("processing_time"))},
        "stats": {"num_segments": int(result.get("num_segments", 0))},
    }
    if result.get("export_sample_rate") is not None:                                      # `output.sample_rate` was set
        manifest["export"] = {"sr": result["export_sample_rate"], "source_sr": result.get("source_sample_rate"),
                              "cuts_samples": result.get("export_cut_points_samples", [])}
    if result.get("export_format") is not None:                                           # `output.format` was not `wav`
        manifest["export_format"] = result["export_format"]
    if result.get("segment_finish") is not None:                                          # fades / normalisation were on
        manifest["finish"] = result["segment_finish"]
    if result.get("note"):
        manifest["note"] = result["note"]
    for block in ("lyrics_alignment", "boundary_detection", "auto_profile", "intent"):
        if result.get(block) is not None:
            manifest[block] = result[block]
    gpu = {k: result[k] for k in result if str(k).startswith("gpu_pipeline_")}
    if gpu:
        manifest["gpu"] = gpu
    manifest["qa_report"] = build_qa_report(manifest)
    if result.get("bpm") is not None or result.get("method") == "smart_segment_v2":       # `librosa_onset` results, passed through
        manifest["smart_segmentation"] = {"method": result.get("method"), "bpm": result.get("bpm"),
                                          "bar_duration_s": result.get("bar_duration_s"), "density": result.get("density"),
                                          "silence_boundaries": result.get("silence_boundaries", [])}
    if str(mode) == "hybrid_mdd" and result.get("success"):                               # `hybrid_mdd` results, passed through
        for key in ("segment_lib_flags", "lib_segment_count", "hybrid_config", "beat_analysis", "strategy"):
            manifest[key] = result.get(key)
    return manifest


__all__ = ["separate_and_segment", "load_audio_mono", "load_audio_stereo", "load_audio_device", "last_result"]
