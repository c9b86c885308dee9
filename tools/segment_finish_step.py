"""What segment finishing costs (`quality_control.fade_in_duration`, `fade_out_duration`, `normalize_audio`), in one process.

    python tools/segment_finish_step.py [--steps 20] [--warmup 3] [--seconds 240] [--log profiles/segment_finish_measure.log]

Track: the seeded `signals.c2_song(seconds, seed=2)` as the mix and two seeded stems of the same length, resident on the device and
on the host as `_split_and_export` has them after `split_track`; 8 s segments (30 for four minutes).  No U-Net runs here.

(1) The pack kernels between device events, alternated: `acf_pack_spans` with fades (441, 441) and gains of 0.5, with fades (0, 0)
    and gains of 1, and `ac_pack_pcm`, on the mono track and on a stereo one, PCM_24 and FLOAT.  All three move the same bytes
    (4 read + width written per word); the achieved bytes/s and the ratio to `ac_pack_pcm` are reported.  `acf_span_stats` alone
    likewise.  The span tables are uploaded once, outside the timed region: the kernels are what is compared.
(2) The export phase as `_split_and_export` runs it with the full plan (mix segments, vocal segments, both full stems written under
    a temporary directory), host clock between two device synchronisations, alternated: `off` (no key set), `off again` (the same
    call a second time per round: the spread of one code path beside itself), `fades`, `fades+normalize`.  With the keys set the
    vocal stem is converted twice (finished for the segments, plain for the full file) and the stats launch and its download of
    n_spans * 16 partials come on top.
(3) The gate `api._configured_finish` at the defaults, the only thing a run without the keys executes of this feature: host
    microseconds per call.
Every line of the log is one JSON object: median, min and max, and the runs."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--log", default="profiles/segment_finish_measure.log")
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native, api
    from audio_cut_amd._finish_native import FinishKernels
    from audio_cut_amd.testing import signals
    from audio_cut_amd.utils import segment_finish as SF
    from audio_cut_amd.utils.audio_export import PackedTrack, SegmentExporter, subtype_info

    sr = 44100
    hip = _native.Context("cuda:0")
    kernels = FinishKernels(hip)
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
    lines = []

    def emit(obj) -> None:
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def stats(v, digits=3):
        return {"median": round(float(np.median(v)), digits), "min": round(float(np.min(v)), digits),
                "max": round(float(np.max(v)), digits), "runs": [round(float(t), digits) for t in v]}

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    # (1) the kernels
    starts = hip.to_device(np.array([lo for lo, _ in spans], dtype=np.int64))
    ends = hip.to_device(np.array([hi for _, hi in spans], dtype=np.int64))
    half = hip.to_device(np.full(len(spans), 0.5, dtype=np.float32))
    ones = hip.to_device(np.ones(len(spans), dtype=np.float32))
    stream = _native._stream
    tracks = {1: dev["mix"], 2: torch.stack([dev["mix"], dev["vocal"]]).contiguous()}
    emit({"measure": "pack_kernel", "frames": n, "spans": len(spans), "steps": a.steps, "warmup": a.warmup})
    for ch, xd in tracks.items():
        for subtype in ("PCM_24", "FLOAT"):
            code, width = subtype_info(subtype)
            out = torch.empty(n * ch * width, dtype=torch.uint8, device=hip.device)
            stride = int(xd.stride(0)) if ch == 2 else n

            def spans_call(gain, fi, fo):
                rc = kernels.lib.acf_pack_spans(xd.data_ptr(), n, ch, stride, starts.data_ptr(), ends.data_ptr(), gain.data_ptr(),
                                                len(spans), fi, fo, code, out.data_ptr(), stream())
                assert rc == 0

            variants = {"ac_pack_pcm": lambda: hip.pack_pcm_device(xd, subtype, out=out),
                        "acf_pack_spans (441, 441)": lambda: spans_call(half, 441, 441),
                        "acf_pack_spans (0, 0)": lambda: spans_call(ones, 0, 0)}
            ms = {k: [] for k in variants}
            for k in range(a.steps + a.warmup):
                for name, fn in variants.items():
                    t = events(fn)
                    if k >= a.warmup:
                        ms[name].append(t)
            moved = n * ch * (4 + width)
            base = float(np.median(ms["ac_pack_pcm"]))
            for name in variants:
                med = float(np.median(ms[name]))
                emit({"measure": "pack_kernel", "channels": ch, "subtype": subtype, "kernel": name, "bytes_moved": moved,
                      "GB_per_s": round(moved / med / 1e6, 1), "ratio_to_ac_pack_pcm": round(med / base, 3), "ms": stats(ms[name], 4)})
        ss = torch.empty((len(spans), 16), dtype=torch.float64, device=hip.device)
        pk = torch.empty((len(spans), 16), dtype=torch.float32, device=hip.device)
        stride = int(xd.stride(0)) if ch == 2 else n
        t_stats = []
        for k in range(a.steps + a.warmup):
            t = events(lambda: kernels.lib.acf_span_stats(xd.data_ptr(), n, ch, stride, starts.data_ptr(), ends.data_ptr(), len(spans),
                                                          441, 441, ss.data_ptr(), pk.data_ptr(), stream()))
            if k >= a.warmup:
                t_stats.append(t)
        emit({"measure": "stats_kernel", "channels": ch, "bytes_read": 4 * n * ch,
              "GB_per_s": round(4 * n * ch / float(np.median(t_stats)) / 1e6, 1), "ms": stats(t_stats, 4)})

    # (2) the export phase
    tmp_dir = tempfile.TemporaryDirectory(prefix="segment_finish_step_")
    tmp = Path(tmp_dir.name)
    exporter = SegmentExporter(sr)
    subtype = "PCM_24"
    settings = {"off": None, "off again": None,
                "fades": SF.finish_settings({"fade_in_duration": 0.01, "fade_out_duration": 0.01}, sr),
                "fades+normalize": SF.finish_settings({"fade_in_duration": 0.01, "fade_out_duration": 0.01, "normalize_audio": True}, sr)}

    def export_phase(finish, out: Path) -> int:
        kw = lambda k: dict(hip=hip, dev=dev[k])
        if finish is None:
            mix_pk = PackedTrack(host["mix"], sr, subtype, **kw("mix"))
        else:
            mix_pk = PackedTrack.finished(host["mix"], sr, spans, finish, subtype, **kw("mix"))
        files = exporter.export_spans(mix_pk, spans, str(out), segment_is_vocal=flags)
        voc_pk = PackedTrack(host["vocal"], sr, subtype, **kw("vocal"))
        seg_pk = voc_pk if finish is None else PackedTrack.finished(host["vocal"], sr, spans, finish, subtype, **kw("vocal"))
        files += exporter.export_spans(seg_pk, spans, str(out), segment_is_vocal=flags, subdir="segments_vocal", file_suffix="_vocal")
        files.append(exporter.export_full_track(voc_pk, out / "vocal_full"))
        files.append(exporter.export_full_track(PackedTrack(host["inst"], sr, subtype, **kw("inst")), out / "instrumental"))
        return sum(Path(f).stat().st_size for f in files)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0, r

    ms = {name: [] for name in settings}
    size = {}
    for k in range(a.steps + a.warmup):
        for name, finish in settings.items():
            t, size[name] = timed(lambda: export_phase(finish, tmp / name.replace(" ", "_").replace("+", "_")))
            if k >= a.warmup:
                ms[name].append(t)
    emit({"measure": "export_phase", "track_s": a.seconds, "frames": n, "segments": len(spans), "files": 2 * len(spans) + 2,
          "subtype": subtype, "steps": a.steps, "warmup": a.warmup})
    for name in settings:
        emit({"measure": "export_phase", "variant": name, "bytes_written": size[name], "ms": stats(ms[name]),
              "minus_off_ms": round(float(np.median(ms[name]) - np.median(ms["off"])), 3)})
    same = all((tmp / "off" / p.relative_to(tmp / "off_again")).read_bytes() == p.read_bytes() for p in (tmp / "off_again").rglob("*.wav"))
    full_same = all((tmp / "off" / f"{f}.wav").read_bytes() == (tmp / "fades_normalize" / f"{f}.wav").read_bytes()
                    for f in ("vocal_full", "instrumental"))
    emit({"measure": "export_phase", "off_files_equal": bool(same), "full_files_of_finished_run_equal_off": bool(full_same)})
    tmp_dir.cleanup()

    # (3) the gate at the defaults
    gate = []
    for _ in range(a.steps + a.warmup):
        t0 = time.perf_counter()
        for _ in range(100):
            assert api._configured_finish(sr) is None
        gate.append((time.perf_counter() - t0) * 1e6 / 100)
    emit({"measure": "gate_at_defaults", "us_per_call": stats(gate[a.warmup:])})
    Path(a.log).parent.mkdir(parents=True, exist_ok=True)
    Path(a.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
