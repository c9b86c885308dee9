"""What mode `vpbd_asr` adds, alternating in one process after a warm-up, a host clock between two device synchronisations:

    python tools/vpbd_asr_step.py [--steps 5] [--warmup 1] [--seconds 240] [--mode-steps 5]

  * `copy_ms`: a resident stem of `signals.c2_song(seconds, seed=2)`'s length, 44.1 kHz -> 16 kHz: `fused` = `resample_poly_pcm16`;
    `staged` = `resample_poly` + float32 download + `pcm_bytes_host(.., "PCM_16")`; `float_kernel` = `resample_poly` alone;
  * `track_ms`: one splitter kept, `split_track` of `vpbd_asr` (a `lyrics_case(2, seconds)` timeline through the `fake` provider)
    beside `vpbd_acoustic`.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/vpbd_asr_step.py --mode-steps 0` the kernel statistics
give k_resample_poly_pcm16 beside k_resample_poly at the same shape."""
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mode-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=240.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native, config as cfg
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.testing import signals
    from audio_cut_amd.testing.lyrics_cases import lyrics_case
    from audio_cut_amd.utils.audio_export import pcm_bytes_host

    sr = 44100
    mix = signals.c2_song(a.seconds, seed=2).astype(np.float32)
    hip = _native.Context("cuda:0")

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    stem = hip.to_device(mix)                      # any resident track of the stem's length: the kernel's time does not depend on the values
    out = {}
    copies = {
        "fused": lambda: out.__setitem__("fused", hip.resample_poly_pcm16(stem, 16000, sr)),
        "staged": lambda: out.__setitem__("staged", pcm_bytes_host(hip.resample_poly(stem, 16000, sr).cpu().numpy(), "PCM_16")[0].view("<i2")),
        "float_kernel": lambda: hip.resample_poly(stem, 16000, sr),
    }
    copy_ms = {k: [] for k in copies}
    for k in range(a.steps + a.warmup):
        for name, fn in copies.items():
            t = timed(fn)
            if k >= a.warmup:
                copy_ms[name].append(t)
    same = bool(np.array_equal(out["fused"], out["staged"]))

    track_ms = {"vpbd_asr": [], "vpbd_acoustic": []}
    counts = {}
    if a.mode_steps:
        backend = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip)
        backend.load_model()
        sp = SeamlessSplitter(sr, separator=EnhancedVocalSeparator(sr, backend=backend))
        tmp_dir = tempfile.TemporaryDirectory(prefix="vpbd_asr_step_")
        fixture = Path(tmp_dir.name) / "timeline.json"
        fixture.write_text(json.dumps(lyrics_case(2, a.seconds), ensure_ascii=False), encoding="utf-8")
        on = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "fake", "lyrics_alignment.fixture_path": str(fixture)}

        def run(mode: str):
            def go():
                saved = cfg.snapshot()
                cfg.set_runtime_config(on if mode == "vpbd_asr" else {})
                try:
                    res = sp.split_track(mix, mode=mode)
                finally:
                    cfg.restore(saved)
                counts[mode] = dict(res["boundary_detection"]["candidate_counts"], actual_mode=res["boundary_detection"]["actual_mode"],
                                    words=res["lyrics_alignment"]["word_count"], cuts=len(res["cuts_samples"]))
            return go
        for k in range(a.mode_steps + a.warmup):
            for mode in track_ms:
                t = timed(run(mode))
                if k >= a.warmup:
                    track_ms[mode].append(t)
        tmp_dir.cleanup()

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(t), 3) for t in v]} if v else None
    med = lambda v: float(np.median(v))
    print(json.dumps({
        "track_s": a.seconds, "samples_in": int(stem.numel()), "samples_out": int(out["fused"].size), "steps": a.steps, "mode_steps": a.mode_steps,
        "warmup": a.warmup, "copy_ms": {k: stats(v) for k, v in copy_ms.items()}, "copy_bytes_identical": same,
        "fused_minus_staged_ms": med(copy_ms["fused"]) - med(copy_ms["staged"]),
        "fused_minus_float_kernel_ms": med(copy_ms["fused"]) - med(copy_ms["float_kernel"]),
        "track_ms": {k: stats(v) for k, v in track_ms.items()},
        "vpbd_asr_minus_vpbd_acoustic_ms": (med(track_ms["vpbd_asr"]) - med(track_ms["vpbd_acoustic"])) if a.mode_steps else None,
        "counts": counts}))


if __name__ == "__main__":
    main()
