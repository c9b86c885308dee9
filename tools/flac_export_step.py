"""What the export phase costs with `output.format: flac` beside `wav`, in one process.

    python tools/flac_export_step.py [--steps 7] [--warmup 2] [--seconds 240] [--log profiles/flac_export_measure.log]

Track, plan and clock are those of tools/export_subtype_step.py: the seeded `signals.c2_song(seconds, seed=2)` as the mix and two
seeded stems of the same length, resident on the device and on the host as `_split_and_export` has them after `split_track`; the
full export plan (mix segments and vocal segments in 8 s pieces, the two full stems) written under a temporary directory; host
clock between two device synchronisations, the variants alternated, `--steps` runs each after `--warmup`.

(1) The export phase: `wav PCM_24` (the path of a build without FLAC), `wav PCM_24 again` (the spread of one code path beside
    itself), `wav PCM_16`, `flac PCM_24`, `flac PCM_16`, and `flac PCM_24 md5` (which downloads the PCM bytes as well).  Bytes
    written per variant.  Nothing is decoded here: tests/test_flac_export_gpu.py holds the files against the WAV run's samples.
(2) The two launches (`acl_flac_plan`, `acl_flac_write`) between device events, per track of the plan and subtype, with the
    frames and the compressed bytes of the call.
The track is synthetic (harmonic stacks plus noise hats): its compression ratio says little about music.
Every line of the log is one JSON object: median, min and max in ms, and the runs."""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--log", default="profiles/flac_export_measure.log")
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native
    from audio_cut_amd._flac_native import FlacKernels
    from audio_cut_amd.testing import signals
    from audio_cut_amd.utils.audio_export import PackedTrack, SegmentExporter

    sr = 44100
    hip = _native.Context("cuda:0")
    mix = signals.c2_song(a.seconds, seed=2).astype(np.float32)
    n = mix.shape[-1]
    rng = np.random.default_rng(7)
    vocal = (0.5 * mix + 0.05 * rng.standard_normal(n)).astype(np.float32)
    inst = mix - vocal
    host = {"mix": mix, "vocal": vocal, "inst": inst}
    dev = {k: hip.to_device(v) for k, v in host.items()}
    piece = 8 * sr
    spans = [(lo, min(n, lo + piece)) for lo in range(0, n, piece)]
    flags = [True] * len(spans)
    tmp_dir = tempfile.TemporaryDirectory(prefix="flac_export_step_")
    tmp = Path(tmp_dir.name)
    exporter = SegmentExporter(sr)
    lines = []

    def emit(obj) -> None:
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                "runs": [round(float(t), 3) for t in v]}

    def export_phase(subtype: str, flac, out: Path) -> int:
        kw = lambda k: dict(hip=hip, dev=dev[k], **({} if flac is None else {"flac": flac}))
        mix_pk = PackedTrack(host["mix"], sr, subtype, **kw("mix"))
        files = exporter.export_spans(mix_pk, spans, str(out), segment_is_vocal=flags)
        voc_pk = PackedTrack(host["vocal"], sr, subtype, **kw("vocal"))
        voc_pk.prepare(spans + [(0, n)])            # as `_split_and_export`: the segments and the full stem in one encoder call
        files += exporter.export_spans(voc_pk, spans, str(out), segment_is_vocal=flags, subdir="segments_vocal", file_suffix="_vocal")
        files.append(exporter.export_full_track(voc_pk, out / "vocal_full"))
        files.append(exporter.export_full_track(PackedTrack(host["inst"], sr, subtype, **kw("inst")), out / "instrumental"))
        return sum(Path(f).stat().st_size for f in files)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0, r

    def opts(subtype, md5=False):
        return {"subtype": subtype, "block_size": 4096, "md5": md5}

    variants = [("wav PCM_24", "PCM_24", None), ("wav PCM_24 again", "PCM_24", None), ("wav PCM_16", "PCM_16", None),
                ("flac PCM_24", "PCM_24", opts("PCM_24")), ("flac PCM_16", "PCM_16", opts("PCM_16")),
                ("flac PCM_24 md5", "PCM_24", opts("PCM_24", True))]
    ms = {name: [] for name, _, _ in variants}
    size = {}
    for k in range(a.steps + a.warmup):
        for name, subtype, flac in variants:
            t, size[name] = timed(lambda: export_phase(subtype, flac, tmp / name.replace(" ", "_")))
            if k >= a.warmup:
                ms[name].append(t)
    emit({"measure": "export_phase", "track_s": a.seconds, "frames": n, "segments": len(spans), "files": 2 * len(spans) + 2,
          "steps": a.steps, "warmup": a.warmup})
    for name, _, _ in variants:
        emit({"measure": "export_phase", "variant": name, "bytes_written": size[name], "ms": stats(ms[name])})
    tmp_dir.cleanup()

    # (2) the two launches between device events
    kernels = FlacKernels(hip)
    kernels.timed = True
    calls = {"mix": spans, "vocal": spans + [(0, n)], "inst": [(0, n)]}
    emit({"measure": "flac_launches", "frames": n, "block_size": 4096, "steps": a.steps, "warmup": a.warmup})
    for subtype, width in (("PCM_24", 3), ("PCM_16", 2)):
        pcm = {k: hip.pack_pcm_device(dev[k], subtype) for k in dev}
        ev = {k: ([], []) for k in calls}
        out_bytes, rows = {}, {}
        for step in range(a.steps + a.warmup):
            for k, sp in calls.items():
                stream, files = kernels.encode_device(pcm[k], n, 1, width, sr, sp, 4096)
                out_bytes[k], rows[k] = int(stream.numel()), sum(-(-(hi - lo) // 4096) for lo, hi in sp)
                if step >= a.warmup:
                    ev[k][0].append(kernels.last_ms[0]); ev[k][1].append(kernels.last_ms[1])
        for k, sp in calls.items():
            emit({"measure": "flac_launches", "subtype": subtype, "track": k, "files": len(sp), "frames_coded": rows[k],
                  "pcm_bytes": sum(hi - lo for lo, hi in sp) * width, "flac_bytes": out_bytes[k],
                  "plan_ms": stats(ev[k][0]), "write_ms": stats(ev[k][1])})
    Path(a.log).parent.mkdir(parents=True, exist_ok=True)
    Path(a.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
