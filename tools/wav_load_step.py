"""What loading a WAV costs: the host decode the loader had (`wave` + numpy + upload) beside `api.load_audio_device` (the file's
bytes into pinned memory, one asynchronous copy, one `ac_decode_pcm`), alternated in one process after a warm-up.

    python tools/wav_load_step.py [--steps 10] [--warmup 1] [--seconds 240] [--log profiles/wav_decode_measure.log]

Files: made from a seed in a temporary directory, 44.1 kHz, `--seconds` long (240 s = 10 584 000 frames): s16 stereo, s24 stereo
plain and WAVE_FORMAT_EXTENSIBLE, f32 stereo, s24 mono.  They are read once before the timing, so they sit in the page cache.
Per file and per `audio.channels` (1: the channel mean; 2: planar, for the stereo files), `--steps` times each:
  (a) the former loader: `wave.open` + the numpy arithmetic (copied below as it was) + `Context.to_device` of the float32 track,
      ending in a device synchronise.  `wave` reads format tag 1 alone, so the extensible and the float file have no (a);
  (b) `load_audio_device(path, hip, channels)`, ending in a stream synchronise;
  (b+host) (b) and the download of the decoded track (`.cpu().numpy()`), which `_split_and_export` needs as well: like (a) it ends
      with the track both on the device and on the host;
  (b pageable) (b)'s steps with the bytes read into pageable memory and uploaded synchronously: what pinned staging was chosen against.
And `ac_decode_pcm` alone between two device events on the resident bytes, with the bytes it moves (file bytes in, float32 out)
over that time.  Every line of the log is one JSON object: median, min and max in ms, and the runs.  A format's device path counts
as faster where the median of (b+host) lies below the minimum of (a)."""
from __future__ import annotations

import argparse
import json
import struct
import sys
import tempfile
import time
import wave
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

KS_TAIL = bytes.fromhex("000000001000800000AA00389B71")


def former_read_wav(p):
    """The loader's `_read_wav` before the RIFF reader, kept here as the baseline."""
    import numpy as np
    with wave.open(str(p), "rb") as w:
        sr, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        data = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        data = v.astype(np.float32) / 8388608.0
    elif width == 4:
        data = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"unsupported WAV sample width {width}")
    return data.reshape(-1, ch), sr


def former_load(p, channels):
    """`load_audio_mono` / `load_audio_stereo` as they were, on `former_read_wav`."""
    import numpy as np
    data, sr = former_read_wav(p)
    if channels == 1:
        return (np.mean(data, axis=1).astype(np.float32) if data.shape[1] > 1 else data[:, 0].copy()), sr
    arr = data.T
    if arr.shape[0] == 1:
        arr = np.concatenate([arr, arr], axis=0)
    return np.ascontiguousarray(arr, dtype=np.float32), sr


def wav_blob(tag, channels, rate, width, payload, extensible=False):
    ba = channels * width
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * ba, ba, 8 * width)
    if extensible:
        body += struct.pack("<HHI", 22, 8 * width, 0) + struct.pack("<H", tag) + KS_TAIL
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + b"data" + struct.pack("<I", len(payload))
    return b"RIFF" + struct.pack("<I", 4 + len(chunks) + len(payload)) + b"WAVE" + chunks, payload


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default=str(Path(__file__).resolve().parent.parent / "profiles" / "wav_decode_measure.log"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native, api
    from audio_cut_amd.utils import wav_reader as WR

    sr = 44100
    n = int(round(a.seconds * sr))
    rng = np.random.default_rng(a.seed)
    tmp_dir = tempfile.TemporaryDirectory(prefix="wav_load_step_")
    tmp = Path(tmp_dir.name)
    s16 = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    files = {}
    for name, tag, ch, width, payload, ext in (
            ("s16_stereo", 1, 2, 2, s16.astype("<i2").tobytes(), False),
            ("s24_stereo", 1, 2, 3, rng.integers(0, 256, size=n * 6, dtype=np.uint8).tobytes(), False),
            ("s24_stereo_extensible", 1, 2, 3, rng.integers(0, 256, size=n * 6, dtype=np.uint8).tobytes(), True),
            ("f32_stereo", 3, 2, 4, (s16.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes(), False),
            ("s24_mono", 1, 1, 3, rng.integers(0, 256, size=n * 3, dtype=np.uint8).tobytes(), False)):
        head, payload = wav_blob(tag, ch, sr, width, payload, ext)
        files[name] = tmp / f"{name}.wav"
        with open(files[name], "wb") as fh:
            fh.write(head)
            fh.write(payload)
        files[name].read_bytes()                                         # into the page cache
    del s16

    hip = _native.Context("cuda:0")
    log = Path(a.log)
    log.parent.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.current_stream().synchronize()
        return (time.perf_counter() - t0) * 1000.0

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                "runs": [round(float(t), 2) for t in v]} if v else None

    emit({"tool": "wav_load_step", "frames": n, "seconds": a.seconds, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)})
    for name, path in files.items():
        info = WR.read_wav_info(path)
        has_former = info.sample_format in ("s16", "s24", "s32") and "extensible" not in name
        for channels in ((1, 2) if info.channels == 2 else (1,)):
            def run_a():
                audio, _ = former_load(path, channels)
                if channels == 2:
                    torch.stack([hip.to_device(audio[c]) for c in range(2)])
                else:
                    hip.to_device(audio)
            def run_pageable():
                raw = torch.from_numpy(WR.read_wav_bytes(path, info)).to(hip.device)
                hip.decode_pcm(raw, info, WR.LAYOUT_PLANAR if channels == 2 else WR.LAYOUT_MONO)
            variants = {"a_former_host": run_a if has_former else None,
                        "b_device": lambda: api.load_audio_device(str(path), hip, channels),
                        "b_device_plus_host_copy": lambda: api.load_audio_device(str(path), hip, channels)[0].cpu().numpy(),
                        "b_device_pageable": run_pageable}
            ms = {k: [] for k, fn in variants.items() if fn is not None}
            for k in range(a.steps + a.warmup):
                for key in ms:
                    t = timed(variants[key])
                    if k >= a.warmup:
                        ms[key].append(t)
            row = {"file": name, "format": info.sample_format, "file_channels": info.channels, "audio_channels": channels,
                   "data_bytes": info.data_bytes, **{k: stats(v) for k, v in ms.items()}}
            if has_former:
                row["device_faster_than_spread_of_a"] = bool(np.median(ms["b_device_plus_host_copy"]) < np.min(ms["a_former_host"]))
            else:
                row["a_former_host"] = "none: the `wave` module refuses this file"
            emit(row)
        # the kernel alone, on the resident bytes
        raw_dev = torch.from_numpy(WR.read_wav_bytes(path, info)).to(hip.device)
        for layout in ((WR.LAYOUT_MONO, WR.LAYOUT_PLANAR) if info.channels > 1 else (WR.LAYOUT_MONO,)):
            out_floats = info.n_frames * (info.channels if layout == WR.LAYOUT_PLANAR else 1)
            out = torch.empty(out_floats, dtype=torch.float32, device=hip.device)
            count = torch.empty(1, dtype=torch.int64, device=hip.device)
            ker = []
            for k in range(a.steps + a.warmup):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _native._check(hip.lib.ac_decode_pcm(hip._h, raw_dev.data_ptr(), info.n_frames, info.channels, info.format_code, layout,
                                                     out.data_ptr(), info.n_frames, count.data_ptr(), _native._stream()))
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    ker.append(e0.elapsed_time(e1))
            moved = info.data_bytes + 4 * out_floats
            emit({"file": name, "kernel": "ac_decode_pcm", "layout": "planar" if layout else "mono", "bytes_moved": moved,
                  "ms": stats(ker), "GB_per_s_at_median": round(moved / (float(np.median(ker)) * 1e-3) / 1e9, 1)})
        del raw_dev
    tmp_dir.cleanup()
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
