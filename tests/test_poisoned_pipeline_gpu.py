"""The modes end to end under poisoned allocations (tests/poison_alloc.py): one short seeded track per mode is split unpoisoned, with
every `torch.empty` of the binding layer, the separator, the backend and the chunk VAD filled with 0xFF, and with 0x7F, each
allocation between 4 KiB guard bands; cuts, boundaries, flags, labels, bar and beat lists, the SHA-1 of every stem and of every
exported PCM buffer and the stems' finiteness must be the same in all three runs, and every guard intact.  A kernel that reads
memory nobody wrote, accumulates into memory it assumes clear, or leaves part of an output to whatever the block held before, is
right in a fresh process and wrong in a long-lived one: here it differs between the runs.

Modes with seeded stems use the `_SeededStems` stand-in of tests/test_smart_segment_gpu.py (its stems are plain `hip.to_device`
tensors: they are not under test); the rest runs the real MDX23HipBackend on seeded synthetic weights at its default items per
forward.  Tracks are `signals.c2_song` of 14 and 24 s, the lengths of the existing end-to-end tests."""
import hashlib
import json

import numpy as np
import pytest

import poison_alloc as PA
from audio_cut_amd.testing import signals

pytestmark = pytest.mark.gpu

SR = 44100
COMPARED = ("success", "mode", "method", "note", "cuts_samples", "sample_boundaries", "refine_boundaries", "segment_vocal_flags",
            "segment_lib_flags", "segment_spans", "segment_layout_applied", "num_pauses", "vpbd_selected_times", "bpm", "bar_duration_s",
            "bar_types", "bar_energies", "bar_times", "beat_times", "bar_spectral_centroids", "bar_spectral_bandwidths", "silence_boundaries",
            "density", "strategy", "strategy_cut_points_samples", "strategy_lib_flags", "mdd_cut_points_samples", "refined_lib_flags",
            "quiet_gate", "beat_analysis", "intent", "auto_profile", "guard_adjustments", "guard_shift_stats", "separation_confidence",
            "backend_used")
STEMS = ("vocal_track", "instrumental_track", "vocal_track_stereo", "instrumental_track_stereo", "mono_mix")


def _sha1(a) -> str:
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digest(res: dict) -> dict:
    """What is compared of a `split_track` result: every decision as text (floats by their repr, so bit for bit), the stems and the
    exported sample bytes by SHA-1, the stems' finiteness."""
    out = {k: json.dumps(res[k], sort_keys=True, default=lambda o: o.tolist() if hasattr(o, "tolist") else repr(o)) for k in COMPARED if k in res}
    for k in STEMS:
        if res.get(k) is not None:
            out[k] = (_sha1(res[k]), str(res[k].dtype), tuple(res[k].shape), bool(np.isfinite(res[k]).all()))
    pcm = res.get("stem_pcm24")
    if pcm is not None:
        out["stem_pcm24"] = {k: (_sha1(v), len(v)) if isinstance(v, np.ndarray) else v for k, v in pcm.items()}
    return out


@pytest.fixture
def run_three(hip_ctx):
    return lambda fn: PA.run_three(hip_ctx, fn)


@pytest.fixture(scope="module")
def seeded():
    """(mix, vocal, inst) of tests/test_beat_analysis_gpu.py::test_split_track_beat_analysis_block: 24 s."""
    dur = 24.0
    mix = signals.c2_song(dur, seed=6).astype(np.float32)
    vocal = (signals.voice_with_rests(dur, seed=106)[: len(mix)] * 0.5).astype(np.float32)
    return mix, vocal, (mix - vocal).astype(np.float32)


@pytest.fixture(scope="module")
def backend(hip_ctx):
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    b = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip_ctx)
    b.load_model()
    return b


SEEDED_RUNS = [("v2.2_mdd", {"beat_analysis": True}), ("librosa_onset", {}), ("hybrid_mdd", {}), ("vpbd_acoustic", {}),
               ("vpbd_acoustic", {"smart_cut": True})]


@pytest.mark.parametrize("mode,kwargs", SEEDED_RUNS, ids=[m + "".join(f"-{k}" for k in kw) for m, kw in SEEDED_RUNS])
def test_split_track_with_seeded_stems(hip_ctx, run_three, seeded, mode, kwargs):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    from test_smart_segment_gpu import _SeededStems
    mix, vocal, inst = seeded

    def run(upload):
        splitter = SeamlessSplitter(SR, separator=_SeededStems(hip_ctx, vocal, inst))
        res = splitter.split_track(mix, mode=mode, **kwargs)
        assert res["success"] is True and res["mode"] == mode and len(res["cuts_samples"]) >= 2
        if "beat_analysis" in kwargs:
            assert len(res["beat_analysis"]["bar_energies"]) >= 2
        if "smart_cut" in kwargs:
            assert "intent" in res
        return _digest(res)
    got = run_three(run)
    assert got["vocal_track"][3] and got["instrumental_track"][3]              # finite


def test_vocal_separation_mode(hip_ctx, run_three, backend):
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    song = signals.c2_song(14.0, seed=9).astype(np.float32)                    # tests/test_vocal_separation_gpu.py

    def run(upload):
        res = SeamlessSplitter(SR, separator=EnhancedVocalSeparator(SR, backend=backend)).split_track(song, mode="vocal_separation")
        assert res["success"] is True and res["stem_pcm24"]["n"] == len(song)
        return _digest(res)
    got = run_three(run)
    assert got["stem_pcm24"]["vocal"][1] == 3 * len(song) and got["stem_pcm24"]["vocal"][0] != got["stem_pcm24"]["instrumental"][0]


def test_default_mode_through_the_real_backend(hip_ctx, run_three, backend):
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    song = signals.c2_song(14.0, seed=9).astype(np.float32)

    def run(upload):
        res = SeamlessSplitter(SR, separator=EnhancedVocalSeparator(SR, backend=backend)).split_track(song)
        assert res["success"] is True and res["mode"] == "v2.2_mdd"
        return _digest(res)
    got = run_three(run)
    assert got["vocal_track"][3] and got["instrumental_track"][3]
    assert got["vocal_track"][0] != got["instrumental_track"][0]


@pytest.mark.parametrize("channels", [1, 2])
def test_backend_export_path(hip_ctx, run_three, backend, channels):
    """`separate_track(..., export_pcm24=True)`: the sample bytes of both stems and the energy partials, a mono and a [2, N] track."""
    from audio_cut_amd.utils.gpu_pipeline import ChunkPlan
    song = signals.c2_song(14.0, seed=9, stereo=channels == 2).astype(np.float32)
    n = song.shape[-1]
    half = 7.0
    plans = [ChunkPlan(index=0, start_s=0.0, end_s=half + 0.5, halo_left_s=0.0, halo_right_s=0.5),
             ChunkPlan(index=1, start_s=half - 0.5, end_s=n / float(SR), halo_left_s=0.5, halo_right_s=0.0)]

    def run(upload):
        got = backend.separate_track(upload(song), SR, plans, export_pcm24=True)
        assert (got.channels, got.n) == (channels, n) and got.vocal.numel() == 3 * channels * n
        return {"vocal": _sha1(got.vocal.cpu().numpy()), "instrumental": _sha1(got.instrumental.cpu().numpy()),
                "energy_partials": got.energy_partials, "n_items": got.n_items, "chunk_ranges": got.chunk_ranges}
    got = run_three(run)
    assert got["vocal"] != got["instrumental"] and bool((got["energy_partials"].sum(dim=1) > 0).all())
