"""What the smart-cut intent / AutoProfile layer costs, alternating in one process after a warm-up, a host clock between two device
synchronisations:  python tools/auto_profile_step.py [--steps 7] [--warmup 2] [--seconds 240] [--mode-steps 5]

  * `coverage_ms`: the vocal coverage of a resident stem of `signals.c2_song(seconds, seed=2)`'s length: `device` =
    `Context.vocal_coverage` (three launches + the 16-byte download) and `coverage_from`; `host` = the reference's formula in numpy on
    the same samples (`host_vocal_coverage`, the yardstick); `sweeps_device_ms` = the launches alone between two device events;
  * `track_ms`: one splitter kept, `split_track(mode="vpbd_acoustic")` as it is, with the smart-cut runtime on the default intent, and
    with `segments="many", alignment="beat_lean"` in the configuration; the prefetch entries each run left unused.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/auto_profile_step.py --mode-steps 0` the kernel statistics
give k_profile_peak and k_profile_count on their own."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    for name, kind, default in (("--steps", int, 7), ("--mode-steps", int, 5), ("--warmup", int, 2), ("--seconds", float, 240.0)):
        ap.add_argument(name, type=kind, default=default)
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_cut_amd import _native, config as cfg
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter, host_vocal_coverage
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.testing import signals

    sr = 44100
    mix = signals.c2_song(a.seconds, seed=2).astype(np.float32)
    hip = _native.Context("cuda:0")              # no device: this raises; there is no host stand-in for a measurement
    n = int(mix.size)
    stem = hip.to_device(mix)                    # any resident track of the stem's length: the sweeps' time does not depend on the values
    got = {}

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    def device():
        peak, _, count = hip.vocal_coverage(stem)
        got["device"] = _native.coverage_from(peak, count, n)

    def sweeps() -> float:                       # the launches alone, no download
        out = torch.empty(2, dtype=torch.int64, device=hip.device)
        base = out.data_ptr()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _native._check(hip.lib.ac_abs_peak_coverage(hip._h, stem.data_ptr(), n, 0.03, 1e-5, base, base + 4, base + 8, _native._stream()))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    paths = {"device": device, "host": lambda: got.__setitem__("host", host_vocal_coverage(mix))}
    coverage_ms, sweeps_ms = {k: [] for k in paths}, []
    for k in range(a.steps + a.warmup):
        for name, fn in paths.items():
            coverage_ms[name].append(timed(fn))
        sweeps_ms.append(sweeps())
    coverage_ms = {k: v[a.warmup:] for k, v in coverage_ms.items()}
    sweeps_ms = sweeps_ms[a.warmup:]

    runs = {"plain": ({}, None), "smart_default": ({}, True),
            "smart_many_beat_lean": ({"smart_cut.segments": "many", "smart_cut.alignment": "beat_lean"}, None)}
    track_ms, info = {k: [] for k in runs}, {}
    if a.mode_steps:
        backend = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip)
        backend.load_model()
        sp = SeamlessSplitter(sr, separator=EnhancedVocalSeparator(sr, backend=backend))

        def run(name: str) -> None:
            keys, flag = runs[name]
            saved = cfg.snapshot()
            cfg.set_runtime_config(keys, explicit=False)
            try:
                res = sp.split_track(mix, mode="vpbd_acoustic", smart_cut=flag)
            finally:
                cfg.restore(saved)
            auto = res.get("auto_profile") or {}
            info[name] = {"cuts": len(res["cuts_samples"]), "style": auto.get("style"),
                          "coverage": auto.get("features", {}).get("vocal_coverage_ratio"), "prefetch_unused": hip.prefetch_stats()["unused"]}
        for k in range(a.mode_steps + a.warmup):
            for name in runs:
                t = timed(lambda: run(name))
                if k >= a.warmup:
                    track_ms[name].append(t)

    med = lambda v: float(np.median(v))
    stats = lambda v: {"median": med(v), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(float(t), 3) for t in v]} if v else None
    more = lambda name: (med(track_ms[name]) - med(track_ms["plain"])) if a.mode_steps else None
    print(json.dumps({
        "track_s": a.seconds, "samples": n, "steps": a.steps, "mode_steps": a.mode_steps, "warmup": a.warmup,
        "coverage_ms": {k: stats(v) for k, v in coverage_ms.items()}, "coverage_identical": got["device"] == got["host"],
        "coverage": got["device"], "device_minus_host_ms": med(coverage_ms["device"]) - med(coverage_ms["host"]),
        "sweeps_device_ms": stats(sweeps_ms), "sweeps_bytes": 2 * 4 * n, "sweeps_gb_per_s": 2 * 4 * n / (med(sweeps_ms) * 1e-3) / 1e9,
        "track_ms": {k: stats(v) for k, v in track_ms.items()}, "smart_default_minus_plain_ms": more("smart_default"),
        "smart_many_beat_lean_minus_plain_ms": more("smart_many_beat_lean"), "info": info}))


if __name__ == "__main__":
    main()
