"""What the export phase costs per `output.wav.subtype`, and the `vocal_separation` writer per subtype, in one process.

    python tools/export_subtype_step.py [--steps 7] [--warmup 2] [--seconds 240] [--log profiles/export_subtype_measure.log]

Track: the seeded `signals.c2_song(seconds, seed=2)` as the mix and two seeded stems of the same length, resident on the device and
on the host as `_split_and_export` has them after `split_track`.  No U-Net runs here: the export phase reads finished tracks.

(1) The export phase as `_split_and_export` runs it with the full plan: three `PackedTrack`s (mix, vocal, instrumental: one
    conversion kernel and one download each), the mix segments and the vocal segments (8 s pieces) and the two full stems written
    under a temporary directory.  Host clock between two device synchronisations, the subtypes alternated, `--steps` runs each
    after `--warmup`.  Variants: the six subtypes; `PCM_24 again`, the same call a second time per round (the spread of one code
    path beside itself: every subtype goes through `ac_pack_pcm`); `PCM_16 host`, the conversion PCM_16 had before it
    moved to the device (`pcm_bytes_host` over the host copy of the float track, what `PackedTrack` without a context does).
(2) `ac_mdx_assemble_pcm` (fused: iSTFT waves -> both stems' bytes + energy partials) beside `ac_mdx_assemble_ola` followed by
    `ac_pack_pcm` of both stems (the energy sums left out of the unfused side), between two device events, on a hand-made plan of
    10 s chunks every 7.5 s with 0.5 s halos and seeded waves, per subtype, alternated.
Every line of the log is one JSON object: median, min and max in ms, and the runs."""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SUBTYPES = ("PCM_U8", "PCM_16", "PCM_24", "PCM_32", "FLOAT", "DOUBLE")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--log", default="profiles/export_subtype_measure.log")
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native
    from audio_cut_amd.separation.backends import items_per_chunk
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
    tmp_dir = tempfile.TemporaryDirectory(prefix="export_subtype_step_")
    tmp = Path(tmp_dir.name)
    exporter = SegmentExporter(sr)
    lines = []

    def emit(obj) -> None:
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                "runs": [round(float(t), 3) for t in v]}

    def export_phase(subtype: str, on_device: bool, out: Path) -> int:
        kw = lambda k: dict(hip=hip, dev=dev[k]) if on_device else {}
        mix_pk = PackedTrack(host["mix"], sr, subtype, **kw("mix"))
        files = exporter.export_spans(mix_pk, spans, str(out), segment_is_vocal=flags)
        voc_pk = PackedTrack(host["vocal"], sr, subtype, **kw("vocal"))
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

    variants = [(s, s, True) for s in SUBTYPES] + [("PCM_24 again", "PCM_24", True), ("PCM_16 host", "PCM_16", False)]
    ms = {name: [] for name, _, _ in variants}
    size = {}
    for k in range(a.steps + a.warmup):
        for name, subtype, on_device in variants:
            t, size[name] = timed(lambda: export_phase(subtype, on_device, tmp / name.replace(" ", "_")))
            if k >= a.warmup:
                ms[name].append(t)
    emit({"measure": "export_phase", "track_s": a.seconds, "frames": n, "segments": len(spans), "files": 2 * len(spans) + 2,
          "steps": a.steps, "warmup": a.warmup})
    for name, _, _ in variants:
        emit({"measure": "export_phase", "variant": name, "bytes_written": size[name], "ms": stats(ms[name])})
    same16 = all((tmp / "PCM_16" / p.relative_to(tmp / "PCM_16_host")).read_bytes() == p.read_bytes()
                 for p in (tmp / "PCM_16_host").rglob("*.wav"))
    emit({"measure": "export_phase", "pcm16_device_files_equal_host_files": bool(same16)})
    tmp_dir.cleanup()

    # (2) the vocal_separation writer: fused beside assemble + pack
    chunk, step, halo = 10 * sr, int(7.5 * sr), sr // 2
    ranges = []
    for cs in range(0, n, step):
        ce = min(n, cs + chunk)
        ranges.append((cs, ce, cs + (halo if cs else 0), ce - (halo if ce < n else 0)))
        if ce == n:
            break
    n_it = [items_per_chunk(ce - cs, 4096) for cs, ce, _, _ in ranges]
    base = np.concatenate(([0], np.cumsum(n_it)[:-1])).astype(np.int32)
    col = lambda f: hip.to_device(np.asarray([f(r) for r in ranges], np.int64))
    tables = [col(lambda r: r[0]), col(lambda r: r[1] - r[0]), col(lambda r: r[2]), col(lambda r: r[3]), hip.to_device(base)]
    wave = torch.randn((int(sum(n_it)), 2, 261120), dtype=torch.float32, device=hip.device,
                       generator=torch.Generator(device=hip.device).manual_seed(3)) * 0.3
    xd = dev["mix"]

    def fused(subtype):
        return hip.mdx_assemble_pcm(xd, wave, *tables, subtype)

    def unfused(subtype):
        v, i, _, _ = hip.mdx_assemble_ola(xd, wave, *tables)
        return hip.pack_pcm_device(v, subtype), hip.pack_pcm_device(i, subtype)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    ev = {(s, kind): [] for s in SUBTYPES for kind in ("fused", "assemble+pack")}
    for k in range(a.steps + a.warmup):
        for s in SUBTYPES:
            for kind, fn in (("fused", fused), ("assemble+pack", unfused)):
                t = events(lambda: fn(s))
                if k >= a.warmup:
                    ev[(s, kind)].append(t)
    emit({"measure": "stem_writer", "frames": n, "chunks": len(ranges), "items": int(sum(n_it)), "steps": a.steps, "warmup": a.warmup})
    for s in SUBTYPES:
        emit({"measure": "stem_writer", "subtype": s, "fused_ms": stats(ev[(s, "fused")]), "assemble_pack_ms": stats(ev[(s, "assemble+pack")])})
    Path(a.log).parent.mkdir(parents=True, exist_ok=True)
    Path(a.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
