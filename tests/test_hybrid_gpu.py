"""Mode `hybrid_mdd` on the GPU: `ac_quiet_gate_meansq` against float64 numpy, the gate's decisions and
`split_track(mode="hybrid_mdd")` against the reference's recorded results (tests/golden/hybrid_mdd.npz) with the fixture's seeded
stems and MDD cuts in place of the `v2.2_mdd` run, one track through the real separator, and `separate_and_segment` end to end."""
import json
import types
import wave
from pathlib import Path

import numpy as np
import pytest

from audio_cut_amd import config as cfg
from audio_cut_amd.cutting import hybrid_strategies as HS
from audio_cut_amd.testing import hybrid_cases

pytestmark = pytest.mark.gpu
SR = hybrid_cases.SR
NAMES = [c["name"] for c in hybrid_cases.CASES]


# ---- the kernel against float64 numpy ---------------------------------------------------------------------------------
def _ref_gate(x: np.ndarray, half_win: int, centers):
    n = len(x)
    sq = lambda frame: float(np.mean(np.square(frame, dtype=np.float64)))
    blocks = np.square(x, dtype=np.float64) if half_win == 1 else \
        np.array([sq(x[a:a + half_win]) for a in range(0, n, half_win)], dtype=np.float64)
    count = np.array([max(0, min(n, c + half_win) - max(0, c - half_win)) for c in centers], dtype=np.int64)
    points = np.array([sq(x[max(0, c - half_win):min(n, c + half_win)]) if k > 0 else 0.0 for c, k in zip(centers, count)])
    return blocks, points, count


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.where(ref > 0, ref, 1.0))) if len(ref) else 0.0


@pytest.mark.parametrize("half_win", [1, 64, 3528])
def test_quiet_gate_meansq_against_numpy(hip_ctx, half_win):
    rng = np.random.default_rng(100 + half_win)
    sizes = sorted({s for s in (1, half_win - 1, half_win, half_win + 1, 3 * half_win, 3 * half_win + 1, 3 * SR + 5) if s >= 1})
    for n in sizes:
        x = (rng.standard_normal(n) * 0.2).astype(np.float32)
        if n > 4 * half_win:
            x[2 * half_win: 4 * half_win] = 0.0                                    # digital silence: a block and windows of zeros
        dev = hip_ctx.to_device(x)
        edge = [-half_win - 1, -half_win, -1, 0, half_win, n - 1, n, n + half_win - 1, n + half_win, n + half_win + 1, 3 * half_win]
        centers = np.array(edge + [0, n - 1, n - 1] + rng.integers(-2 * half_win, n + 2 * half_win, size=5000).tolist(), dtype=np.int64)
        blocks, points, count = hip_ctx.quiet_gate(dev, half_win, centers)
        rb, rp, rc = _ref_gate(x, half_win, centers.tolist())
        assert blocks.dtype == points.dtype == np.float64 and count.dtype == np.int64
        assert blocks.shape == rb.shape == (-(-n // half_win),) and np.array_equal(count, rc)
        worst = max(_rel(blocks, rb), _rel(points, rp))
        print(f"quiet_gate half_win={half_win} n={n}: worst relative error {worst:.3e}")
        assert worst <= 1e-12
        assert np.all(points[count == 0] == 0.0) and np.all(points[rp == 0.0] == 0.0) and np.all(blocks[rb == 0.0] == 0.0)
        assert count[0] == 0 and count[8] == 0 and count[9] == 0 and count[3] == min(n, half_win)
        # the window around 0 IS block 0: the same samples in the same order
        assert abs(points[3] * count[3] - blocks[0] * min(n, half_win)) <= 1e-12 * max(blocks[0] * min(n, half_win), 1e-300)
        assert points[3].tobytes() == blocks[0].tobytes()
        again = hip_ctx.quiet_gate(dev, half_win, centers)                         # a fixed order: the same bits on every run
        for a, b in zip((blocks, points, count), again):
            assert a.tobytes() == b.tobytes()
        shuffled = rng.permutation(len(centers))                                   # the order of the centres does not matter
        _, p2, c2 = hip_ctx.quiet_gate(dev, half_win, centers[shuffled])
        assert p2.tobytes() == points[shuffled].tobytes() and np.array_equal(c2, count[shuffled])
        b0, p0, c0 = hip_ctx.quiet_gate(dev, half_win, [])                         # no centres: the blocks alone
        assert b0.tobytes() == blocks.tobytes() and p0.shape == c0.shape == (0,)
    silent = hip_ctx.to_device(np.zeros(3 * half_win + 1, dtype=np.float32))
    b, p, c = hip_ctx.quiet_gate(silent, half_win, [0, half_win, 10 ** 12, -10 ** 12])
    assert np.all(b == 0.0) and np.all(p == 0.0) and c.tolist()[2:] == [0, 0]
    with pytest.raises(ValueError):
        hip_ctx.quiet_gate(silent, 0, [0])


# ---- the mode against the fixture ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "hybrid_mdd.npz")


def _cases(golden):
    return {c["name"]: c for c in json.loads(str(golden["cases"]))}


_BUILT = {}


def _built(case):
    if case["name"] not in _BUILT:
        _BUILT.clear()                                                              # one case's tracks at a time
        _BUILT[case["name"]] = hybrid_cases.build(case)
    return _BUILT[case["name"]]


def _base_for(hip, case, audio, vocal, inst, beats):
    """What `_hybrid_mdd_base` returns, from the case: the listed MDD cuts, the seeded stems resident on the device, the beats."""
    stereo = np.ndim(audio) == 2
    mono = hybrid_cases.mono_of(audio)
    state = {"hip": hip, "mix": hip.to_device(mono), "vocal": hip.to_device(vocal), "instrumental": hip.to_device(inst)}
    base = {"success": bool(case["mdd_success"]), "vocal_track": vocal, "instrumental_track": inst, "device_state": state,
            "feature_cache": types.SimpleNamespace(beat_times=np.asarray(beats, dtype=np.float64), bpm_features=None),
            "gpu_meta": {}, "separation_confidence": 1.0, "backend_used": "seeded", "timings": {"separate_s": 0.0}}
    if case["mdd_success"]:
        base["cuts_samples"] = hybrid_cases.mdd_cut_samples(case, len(mono))
    else:
        base["error"] = "stand-in MDD failure"
    if stereo:
        state["mix_stereo"] = hip.to_device(audio)
        base.update({"mono_mix": mono, "vocal_track_stereo": np.stack([vocal, vocal]), "instrumental_track_stereo": np.stack([inst, inst])})
    return base


def _split(hip, case, audio=None):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    mix, vocal, inst, beats = _built(case)
    audio = mix if audio is None else audio
    stub = types.SimpleNamespace(_primary_backend=types.SimpleNamespace(hip=hip))
    splitter = SeamlessSplitter(SR, separator=stub)
    calls = []
    splitter._hybrid_mdd_base = lambda a, d=None: (calls.append(np.shape(a)), _base_for(hip, case, a, vocal, inst, beats))[1]
    saved = cfg.snapshot()
    cfg.set_runtime_config(dict(case["overrides"]))
    try:
        res = splitter.split_track(audio, mode="hybrid_mdd", hybrid_density=case["density"])
    finally:
        cfg.restore(saved)
    assert calls == [np.shape(audio)]
    return res


def _close(got, want, tol=1e-4, relative=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if got.size:
        err = np.abs(got - want) / (np.abs(want) if relative else 1.0)
        assert float(np.max(err)) <= tol, float(np.max(err))


@pytest.mark.parametrize("name", NAMES)
def test_gate_decisions_match_the_reference(hip_ctx, golden, name):
    case = _cases(golden)[name]
    g = lambda k: golden[f"{name}__{k}"]
    if not len(g("gate_times")):            # forced or unprotected snapping, no chorus: the reference asked the gate nothing
        return
    _, vocal, _, _ = _built(case)
    eff = case["effective_config"]
    half_win = HS.gate_half_window(SR, eff["guard_win_ms"])
    centers = [HS.gate_center(float(t), SR) for t in g("gate_times")]
    assert centers == g("gate_centers").tolist()
    blocks, points, count = hip_ctx.quiet_gate(hip_ctx.to_device(vocal), half_win, centers)
    floor_db, point_db, quiet = HS.gate_decisions(blocks, points, count, eff["guard_db"])
    print(f"{name}: {len(centers)} gated times, floor {floor_db:.6f} dB (reference {float(g('gate_floor_db')[0]):.6f})")
    assert quiet.tolist() == g("gate_quiet").tolist()
    _close(point_db, g("gate_point_db"))
    _close([floor_db] * len(centers), g("gate_floor_db"))


@pytest.mark.parametrize("name", NAMES)
def test_split_track_matches_the_reference(hip_ctx, golden, name):
    case = _cases(golden)[name]
    g = lambda k: golden[f"{name}__{k}"].tolist()
    res = _split(hip_ctx, case)
    n = case["n_samples"]
    assert res["success"] is True and res["mode"] == "hybrid_mdd"
    assert res["method"] == case["method"] == f"hybrid_mdd_{case['strategy']}" and res["strategy"] == case["strategy"]
    assert res["hybrid_config"] == case["hybrid_config"] and res["strategy_metadata"] == case["strategy_metadata"]
    assert res["beat_analysis"]["num_bars"] == case["beat_analysis"]["num_bars"]
    _close([res["beat_analysis"]["bpm"], res["beat_analysis"]["bar_duration_s"]],
           [case["beat_analysis"]["bpm"], case["beat_analysis"]["bar_duration_s"]])
    _close(res["beat_times"], g("beats")); _close(res["bar_times"], g("bar_times"))
    for mine, theirs in (("bar_energies", "bar_energies"), ("bar_spectral_centroids", "bar_centroids"), ("bar_spectral_bandwidths", "bar_bandwidths")):
        _close(res[mine], g(theirs), relative=True)
    # every time the reference asked about was gated here, with its answer
    gate = res["quiet_gate"]
    assert [gate["quiet"][c] for c in g("gate_centers")] == g("gate_quiet")
    assert len(gate["centers"]) == len(set(gate["centers"])) == len(gate["point_db"])
    assert res["mdd_cut_points_samples"] == g("mdd_cuts")
    assert res["strategy_cut_points_samples"] == g("strategy_cuts") and res["strategy_lib_flags"] == g("strategy_flags")
    assert res["sample_boundaries"] == g("refined_cuts") and res["refined_lib_flags"] == g("refined_flags")
    assert res["cuts_samples"] == g("final_cuts") and res["segment_lib_flags"] == g("final_lib_flags")
    assert res["lib_segment_count"] == case["lib_segment_count"] == sum(g("final_lib_flags"))
    assert res["segment_vocal_flags"] == g("final_vocal_flags")
    assert [hi - lo for lo, hi in res["segment_spans"]] == g("span_lengths") and res["segment_spans"][-1][1] == n
    _close(res["segment_durations"], g("segment_durations")); _close(res["cuts_sec"], [c / float(SR) for c in g("final_cuts")])
    assert set(res["timings"]) == {"separate_s", "detect_s", "finalize_s"}
    assert res["guard_shift_stats"]["count"] == len(res["guard_adjustments"]) and isinstance(res["precision_guard_ok"], bool)
    assert res["vocal_track"] is not None and res["device_state"]["vocal"] is not None


def test_split_track_stereo_equals_mono_of_mean(hip_ctx, golden):
    case = _cases(golden)["stereo_input"]
    mix, _, _, _ = _built(case)
    assert mix.ndim == 2
    st = _split(hip_ctx, case)
    mono = _split(hip_ctx, case, audio=hybrid_cases.mono_of(mix))
    for key in ("cuts_samples", "segment_lib_flags", "segment_vocal_flags", "segment_spans", "sample_boundaries", "strategy_cut_points_samples",
                "bar_energies", "strategy_metadata"):
        assert st[key] == mono[key], key
    assert np.array_equal(st["mono_mix"], hybrid_cases.mono_of(mix)) and "mono_mix" not in mono
    assert st["vocal_track_stereo"].shape == (2, mix.shape[1]) and tuple(st["device_state"]["mix_stereo"].shape) == mix.shape


def test_unsupported_combinations_are_refused(hip_ctx, golden):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    splitter = SeamlessSplitter(SR, separator=types.SimpleNamespace(_primary_backend=types.SimpleNamespace(hip=hip_ctx)))
    with pytest.raises(ValueError):
        splitter.split_track(np.zeros(SR, np.float32), mode="hybrid_mdd", separation_gate=object())


# ---- the real separator ------------------------------------------------------------------------------------------------------
def _track_30s():
    mix, _, _, _ = hybrid_cases.build({c["name"]: c for c in hybrid_cases.CASES}["stereo_input"])
    return hybrid_cases.mono_of(mix)


def test_real_separator_runs_once_and_feeds_the_mdd_cuts(hip_ctx):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    mix = _track_30s()
    splitter = SeamlessSplitter(SR)
    real = splitter.separator.separate_for_detection
    calls = []
    splitter.separator.separate_for_detection = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    hyb = splitter.split_track(mix, mode="hybrid_mdd")
    assert len(calls) == 1                                                          # one separation, where the reference runs two
    mdd = splitter.split_track(mix, mode="v2.2_mdd")
    assert len(calls) == 2
    assert hyb["success"] and hyb["mdd_success"] and hyb["mdd_cut_points_samples"] == [int(c) for c in mdd["cuts_samples"]]
    assert hyb["vocal_track"].tobytes() == mdd["vocal_track"].tobytes()
    assert hyb["instrumental_track"].tobytes() == mdd["instrumental_track"].tobytes()
    cuts = hyb["cuts_samples"]
    assert cuts[0] == 0 and cuts[-1] == len(mix) and cuts == sorted(set(cuts))
    assert len(hyb["segment_lib_flags"]) == len(cuts) - 1 and hyb["method"] == "hybrid_mdd_snap_to_beat"
    beats = hyb["beat_times"]
    gated = set(hyb["quiet_gate"]["centers"])
    assert all(HS.gate_center(t, SR) in gated for t in beats + hyb["bar_times"])


def _read_pcm24(path, frames=None):
    with wave.open(str(path), "rb") as w:
        assert (w.getsampwidth(), w.getframerate()) == (3, SR)
        ch, n = w.getnchannels(), w.getnframes()
        raw = np.frombuffer(w.readframes(n if frames is None else frames), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
    v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    return np.where(v & 0x800000, v - 0x1000000, v).reshape(-1, ch) / 8388608.0


def test_separate_and_segment_hybrid_mdd_end_to_end(hip_ctx, tmp_path):
    from audio_cut_amd import api
    mix = _track_30s()
    pcm = np.clip(np.round(mix.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
    src = tmp_path / "song.wav"
    with wave.open(str(src), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())
    loaded = pcm.astype(np.float32) / 32768.0
    out_dir = tmp_path / "out"
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(out_dir), mode="hybrid_mdd", export_manifest=True,
                                   runtime_overrides={"segment_layout.soft_min_s": 1.5})
    res = api.last_result()
    cuts, lib, flags = res["cut_points_samples"], res["segment_lib_flags"], res["segment_vocal_flags"]
    assert man["success"] is True and man["version"] == "hybrid_mdd" and man["cuts"]["samples"] == cuts
    assert man["export_plan"] == ["full_vocal", "mix_segments", "vocal_segments"]
    for key in ("segment_lib_flags", "lib_segment_count", "hybrid_config", "beat_analysis", "strategy"):
        assert man[key] == res[key] and man[key] is not None, key
    assert man["strategy"] == "snap_to_beat" and man["lib_segment_count"] == sum(lib) and len(lib) == len(cuts) - 1
    assert set(man["beat_analysis"]) == {"bpm", "bar_duration_s", "num_bars"}
    assert len(res["mix_segment_files"]) == len(res["vocal_segment_files"]) == len(cuts) - 1 and res["full_instrumental_file"] is None
    vocal_full = out_dir / f"song_hybrid_mdd_vocal_full_{len(loaded) / float(SR):.1f}.wav"
    assert Path(res["full_vocal_file"]).name == vocal_full.name and vocal_full.exists()
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        label = "human" if flags[i] else "music"
        stem = f"segment_{i + 1:03d}_{label}{'_lib' if lib[i] else ''}"
        mix_file, voc_file = res["mix_segment_files"][i], res["vocal_segment_files"][i]
        assert Path(mix_file).name == f"{stem}_{(b - a) / float(SR):.1f}.wav", (i, mix_file)
        assert Path(voc_file).name == f"{stem}_vocal_{(b - a) / float(SR):.1f}.wav" and Path(voc_file).parent.name == "segments_vocal"
        assert ("_lib" in Path(mix_file).name) == bool(lib[i]) == ("_lib" in Path(voc_file).name)
        seg = _read_pcm24(mix_file)[:, 0]
        assert len(seg) == b - a and np.max(np.abs(seg - loaded[a:b])) <= 2.0 ** -23            # the slice at cuts_samples
    full = _read_pcm24(vocal_full)[:, 0]
    pieces = np.concatenate([_read_pcm24(f)[:, 0] for f in res["vocal_segment_files"]])
    assert np.array_equal(pieces, full)                                                         # the vocal segments tile the full vocal
    json.loads((out_dir / "SegmentManifest.json").read_text())
