"""What mode `vocal_separation` costs beside the nearest thing the other modes offer, a `v2.2_mdd` run that exports the two stems
only: both alternated in one process after one warm-up each.

    python tools/vocal_separation_step.py [--steps 3] [--warmup 1] [--seconds 240] [--api-steps 3]

Track: the seeded `signals.c2_song(240, seed=2)` (the benchmark's C2 track), written as a 44.1 kHz PCM_16 WAV.  Two timings, each
a host clock between two device synchronisations:
  * `api_ms`: `separate_and_segment(mode=...)` as a user calls it - it builds its splitter (weights, context) on every call, so
    this is mostly set-up, the same for both modes;
  * `track_ms`: one splitter kept, `split_track` plus writing the two stem files - the per-track work the modes differ in.
Prints one JSON line: median, min and max per mode, the differences of the medians, and whether the files of the two modes hold
the same bytes.  Under `rocprofv3 --kernel-trace --stats -- python tools/vocal_separation_step.py --api-steps 0` the kernel
statistics give k_mdx_assemble_pcm (the PCM_24 instance) beside k_mdx_assemble_ola + k_pack_pcm (its PCM_24 instance) + k_sum_squares."""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
import wave
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--api-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=240.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native, api
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.testing import signals
    from audio_cut_amd.utils.audio_export import PackedTrack, SegmentExporter

    sr = 44100
    mix = signals.c2_song(a.seconds, seed=2)
    tmp_dir = tempfile.TemporaryDirectory(prefix="vocal_separation_step_")
    tmp = Path(tmp_dir.name)
    src = tmp / "c2.wav"
    with wave.open(str(src), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.clip(np.rint(mix * 32767.0), -32768, 32767).astype("<i2").tobytes())
    track, _ = api.load_audio_mono(str(src))
    stems = ["full_vocal", "full_instrumental"]

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    # as a user calls it
    def api_run(mode: str, out: str):
        return lambda: api.separate_and_segment(input_uri=str(src), export_dir=str(tmp / out), mode=mode, export_types=stems)
    api_ms = {"vocal_separation": [], "v2.2_mdd": []}
    for k in range(a.api_steps + (a.warmup if a.api_steps else 0)):
        for mode in api_ms:
            t = timed(api_run(mode, f"api_{mode}"))
            if k >= a.warmup:
                api_ms[mode].append(t)

    # one splitter kept
    hip = _native.Context("cuda:0")
    backend = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip)
    backend.load_model()
    sp = SeamlessSplitter(sr, separator=EnhancedVocalSeparator(sr, backend=backend))
    exporter = SegmentExporter(sr)
    files = {}

    def sep_only():
        res = sp.split_track(track, mode="vocal_separation")
        out = api._export_vocal_separation(res, src, tmp / "track_sep", stems, sr, time.time())
        files["vocal_separation"] = (out["full_vocal_file"], out["full_instrumental_file"])

    def mdd_stems():
        res = sp.split_track(track, mode="v2.2_mdd")
        state = res["device_state"]
        files["v2.2_mdd"] = tuple(
            exporter.export_full_track(PackedTrack(res[f"{kind}_track"], sr, hip=hip, dev=state[kind]), tmp / "track_mdd" / f"c2_{kind}")
            for kind in ("vocal", "instrumental"))
    runs = {"vocal_separation": sep_only, "v2.2_mdd": mdd_stems}
    track_ms = {"vocal_separation": [], "v2.2_mdd": []}
    for k in range(a.steps + a.warmup):
        for mode, fn in runs.items():
            t = timed(fn)
            if k >= a.warmup:
                track_ms[mode].append(t)
    same = all(Path(x).read_bytes() == Path(y).read_bytes() for x, y in zip(files["vocal_separation"], files["v2.2_mdd"]))
    tmp_dir.cleanup()

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(t), 2) for t in v]} if v else None
    diff = lambda d: float(np.median(d["vocal_separation"]) - np.median(d["v2.2_mdd"])) if d["v2.2_mdd"] else None
    print(json.dumps({"track_s": a.seconds, "steps": a.steps, "api_steps": a.api_steps, "warmup": a.warmup,
                      "api_ms": {k: stats(v) for k, v in api_ms.items()}, "api_vocal_separation_minus_v22_ms": diff(api_ms),
                      "track_ms": {k: stats(v) for k, v in track_ms.items()}, "track_vocal_separation_minus_v22_ms": diff(track_ms),
                      "stem_files_identical": bool(same)}))


if __name__ == "__main__":
    main()
