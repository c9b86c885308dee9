"""What true-stereo separation costs per track: mono `split_track` on the channel mean against stereo `split_track` on the
planar (2, N) track, alternated in one process after both are warm.

    python tools/stereo_step.py [--steps 6] [--warmup 1] [--seconds 240]

Track: the seeded `signals.c2_song(240, seed=2, stereo=True)`; full-size TFC-TDF with seeded synthetic weights, 64 items per
forward (the library default).  Prints one JSON line: ms per track for each path (median, min, max over the steps) and the
stereo - mono difference of the medians.  Under `rocprofv3 --kernel-trace --stats -- python tools/stereo_step.py` the kernel
statistics give the per-kernel times (k_mdx_stft<1> vs k_mdx_stft<2>, ...)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=240.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.testing import signals

    sr = 44100
    st = signals.c2_song(a.seconds, seed=2, stereo=True)
    mono = np.mean(st, axis=0).astype(np.float32)
    hip = _native.Context("cuda:0")
    backend = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip)
    backend.load_model()
    sp = SeamlessSplitter(sr, separator=EnhancedVocalSeparator(sr, backend=backend))

    def run(x) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sp.split_track(x)
        torch.cuda.synchronize()
        run.last = res
        return (time.perf_counter() - t0) * 1000.0

    for _ in range(max(0, a.warmup)):
        run(mono); run(st)
    t_mono, t_st = [], []
    stage = {"mono": [], "stereo": []}
    for _ in range(a.steps):
        t_mono.append(run(mono)); stage["mono"].append(run.last["device_state"]["timings"].get("stft_ms", 0.0))
        t_st.append(run(st)); stage["stereo"].append(run.last["device_state"]["timings"].get("stft_ms", 0.0))

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    print(json.dumps({"track_s": a.seconds, "steps": a.steps, "mono_ms": stats(t_mono), "stereo_ms": stats(t_st),
                      "stereo_minus_mono_ms": float(np.median(t_st) - np.median(t_mono)),
                      "stft_stage_ms": {k: stats(v) for k, v in stage.items()}}))


if __name__ == "__main__":
    main()
