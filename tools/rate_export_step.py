"""What `output.sample_rate` costs ("Export rate").

Default: the three export conversions of a 4-min stereo track, 44.1 -> 48 kHz, PCM_24, between device events, alternated, twelve timed
runs after three warm-ups: (a) `ac_resample_poly_pack` for both stems, (b) the composition it replaces, `ac_resample_poly` per
channel into the rows of one planar buffer + `ac_pack_pcm`, for both stems; the mix through `ac_pack_pcm` on either side.  The
bytes of the two sides are compared in the same run.

`--e2e`: wall time of `separate_and_segment` on a seeded 60 s stereo 48 kHz 16-bit file with `output.sample_rate: "source"` and
without it, alternated, five runs each (the first of each is the warm-up)."""
import json
import statistics
import sys
import tempfile
import time
import wave
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def kernels() -> None:
    from audio_cut_amd import _native
    from audio_cut_amd._native import _check, _stream
    from audio_cut_amd.utils import rate_export as RE
    SR, OUT = 44100, 48000
    hip = _native.Context("cuda:0")
    n = 240 * SR
    up, down = RE.rate_ratio(OUT, SR)
    n_out = 240 * OUT
    g = torch.Generator(device="cuda").manual_seed(0)
    vocal = torch.randn((2, n), device=hip.device, generator=g) * 0.3
    inst = torch.randn((2, n), device=hip.device, generator=g) * 0.3
    mix48 = torch.randn((2, n_out), device=hip.device, generator=g) * 0.3
    hd, npr = hip._resample_filter_dev(up, down)
    tmp = torch.empty((2, n_out), dtype=torch.float32, device=hip.device)

    def fused():
        a = RE.resample_pack_device(hip, vocal, up, down, "PCM_24", n_out)
        b = RE.resample_pack_device(hip, inst, up, down, "PCM_24", n_out)
        c = hip.pack_pcm_device(mix48, "PCM_24")
        return a, b, c

    def composed():
        outs = []
        for stem in (vocal, inst):
            for ch in range(2):
                _check(hip.lib.ac_resample_poly(hip._h, stem[ch].data_ptr(), n, up, down, hd.data_ptr(), hd.numel(), npr, tmp[ch].data_ptr(), n_out, _stream()))
            outs.append(hip.pack_pcm_device(tmp, "PCM_24"))
        outs.append(hip.pack_pcm_device(mix48, "PCM_24"))
        return outs

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(3):
        ra, rb = fused(), composed()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ra, rb)), "fused and composed bytes differ"
    ta, tb = [], []
    for _ in range(12):
        ta.append(timed(fused)[0]); tb.append(timed(composed)[0])
    tm = [timed(lambda: hip.pack_pcm_device(mix48, "PCM_24"))[0] for _ in range(12)]
    res = {"n": n, "n_out": n_out, "taps_per_output": hd.numel() // up,
           "fused_ms": {"median": statistics.median(ta), "min": min(ta), "max": max(ta)},
           "composed_ms": {"median": statistics.median(tb), "min": min(tb), "max": max(tb)},
           "mix_pack_ms": {"median": statistics.median(tm), "min": min(tm), "max": max(tm)}, "fused_runs": ta, "composed_runs": tb}
    print(json.dumps(res))


def end_to_end() -> None:
    import scipy.signal
    from audio_cut_amd import api
    from audio_cut_amd.testing import signals
    root = Path(tempfile.mkdtemp())
    st = signals.c2_song(60.0, seed=9, stereo=True)
    st48 = np.stack([scipy.signal.resample_poly(ch, 160, 147) for ch in st]).astype(np.float32)
    src = root / "song48.wav"
    with wave.open(str(src), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(np.clip(np.rint(st48.T * 32767.0), -32768, 32767).astype("<i2").tobytes())
    base = {"audio.channels": 2}
    def run(tag, extra, i):
        t = time.perf_counter()
        api.separate_and_segment(input_uri=str(src), export_dir=str(root / f"{tag}{i}"), runtime_overrides={**base, **extra})
        torch.cuda.synchronize()
        return time.perf_counter() - t
    times = {"plain": [], "source": []}
    for i in range(5):
        times["plain"].append(run("plain", {}, i)); times["source"].append(run("source", {"output.sample_rate": "source"}, i))
    res = {k: {"runs_s": v, "median_after_first_s": statistics.median(v[1:])} for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    end_to_end() if "--e2e" in sys.argv[1:] else kernels()
