"""Mode `librosa_onset` on the GPU: the two kernels of include/audiocut_hip_onset.h against float64 numpy restatements,
`split_track(mode="librosa_onset")` against the reference's recorded results (tests/golden/librosa_onset.npz) with the
fixture's seeded stems in place of the network, and `separate_and_segment` end to end with the real separator."""
import json
import types

import numpy as np
import pytest

from audio_cut_amd import config as cfg
from audio_cut_amd.testing import onset_cases

pytestmark = pytest.mark.gpu
SR = 44100
TYPE_NAME = {0: "verse", 1: "chorus", 2: "chorus_peak"}


# ---- float64 restatements ---------------------------------------------------------------------------------------------
def _bar_means(rms: np.ndarray, lo, hi) -> np.ndarray:
    x = rms.astype(np.float64)
    return np.array([x[a:b].sum() / (b - a) if b > a else 0.0 for a, b in zip(lo, hi)], dtype=np.float64)


def _db(rms: np.ndarray) -> np.ndarray:
    return 20.0 * np.log10(rms.astype(np.float64) + 1e-10)


def _rms_with_margin(rng, n: int, thr_db: float) -> np.ndarray:
    """float32 RMS-like values between -70 and -10 dB, none within 1e-3 dB of the threshold, with exact zeros mixed in."""
    x = (10.0 ** (rng.uniform(-70.0, -10.0, size=n) / 20.0)).astype(np.float32)
    near = np.abs(_db(x) - thr_db) < 1e-3
    x[near] = np.float32(10.0 ** ((thr_db + 1.0) / 20.0))
    x[rng.integers(0, n, size=max(1, n // 50))] = 0.0            # digital silence: -200 dB
    assert np.all(np.abs(_db(x) - thr_db) >= 1e-3)
    return x


def test_bar_energy_silence_against_numpy(hip_ctx):
    rng = np.random.default_rng(11)
    thr = -40.0
    shapes = []
    n = 20672                                                             # a 4-min track at hop 512
    edges = np.sort(rng.integers(0, n, size=121)); edges[0] = 0
    shapes.append((n, edges[:-1], np.append(edges[1:-1], n)))              # ~120 bars, the last one partial up to the end
    shapes.append((n, np.array([0]), np.array([n])))                       # one bar over everything
    shapes.append((n, np.array([5, 100, 100, 700]), np.array([6, 100, 90, 701])))     # 1-frame ranges, an empty and an inverted one
    k = 5000
    lo = rng.integers(0, n - 8, size=k)
    shapes.append((n, lo, lo + rng.integers(0, 8, size=k)))                # several thousand short bars, overlapping, some empty
    shapes.append((1, np.array([0, 0, 1]), np.array([1, 0, 1])))           # a single frame
    shapes.append((257, np.array([0, 256]), np.array([256, 257])))         # one frame past a full workgroup of flags
    for n_frames, lo, hi in shapes:
        rms = _rms_with_margin(rng, n_frames, thr)
        dev = hip_ctx.to_device(rms)
        means, silent = hip_ctx.bar_energy_silence(dev, lo, hi, thr)
        ref = _bar_means(rms, lo, hi)
        assert means.dtype == np.float64 and means.shape == ref.shape
        empty = np.asarray(hi) <= np.asarray(lo)
        assert np.all(means[empty] == 0.0)
        scale = np.where(ref > 0, ref, 1.0)
        worst = float(np.max(np.abs(means - ref) / scale))
        print(f"bar_energy_silence n_frames={n_frames} n_bars={len(lo)}: worst relative error {worst:.3e}")
        assert worst <= 1e-6
        assert silent.dtype == bool and np.array_equal(silent, _db(rms) < thr)
        assert np.all(silent[rms == 0.0])
        means2, silent2 = hip_ctx.bar_energy_silence(dev, lo, hi, thr)       # a fixed order: the same bits every run
        assert np.array_equal(means.view(np.uint64), means2.view(np.uint64)) and np.array_equal(silent, silent2)
    with pytest.raises(ValueError):
        hip_ctx.bar_energy_silence(dev, [0], [n_frames + 1], thr)


def test_segment_pair_energy_against_numpy(hip_ctx):
    rng = np.random.default_rng(12)
    n = 60 * SR
    vocal = (rng.standard_normal(n) * 0.1).astype(np.float32)
    inst = (rng.standard_normal(n) * 0.3 * (0.1 + np.abs(np.sin(np.arange(n) * 1e-5)))).astype(np.float32)
    dv, di = hip_ctx.to_device(vocal), hip_ctx.to_device(inst)
    cuts = np.sort(rng.choice(np.arange(1, n), size=999, replace=False))
    cases = [
        (np.array([0]), np.array([n])),                                    # the whole track, one segment
        (np.array([0, 7, n - 1]), np.array([1, 8, n])),                    # segments of one sample
        (np.concatenate(([0], cuts)), np.concatenate((cuts, [n]))),        # 1000 segments tiling the track
        (np.array([0, 352256, 792576]), np.array([352256, 792576, n])),
    ]
    rel = lambda got, ref: float(np.max(np.abs(got - ref) / np.where(ref > 0, ref, 1.0)))
    for a, b in cases:
        sv, si = hip_ctx.segment_pair_energy(dv, di, a, b)
        rv = np.array([np.sum(vocal[x:y].astype(np.float64) ** 2) for x, y in zip(a, b)])
        ri = np.array([np.sum(inst[x:y].astype(np.float64) ** 2) for x, y in zip(a, b)])
        print(f"segment_pair_energy n_seg={len(a)}: worst relative error vocal {rel(sv, rv):.3e} inst {rel(si, ri):.3e}")
        assert rel(sv, rv) <= 1e-12 and rel(si, ri) <= 1e-12
        # the one-signal kernel twice: the same partial sums
        ov = hip_ctx.segment_sumsq_peak(dv, a, b)[0]
        oi = hip_ctx.segment_sumsq_peak(di, a, b)[0]
        assert np.array_equal(sv.view(np.uint64), ov.view(np.uint64)) or rel(sv, ov) <= 1e-12
        assert np.array_equal(si.view(np.uint64), oi.view(np.uint64)) or rel(si, oi) <= 1e-12
        sv2, si2 = hip_ctx.segment_pair_energy(dv, di, a, b)
        assert np.array_equal(sv.view(np.uint64), sv2.view(np.uint64)) and np.array_equal(si.view(np.uint64), si2.view(np.uint64))
    # no instrumental stem: its sums are zeros, the vocal's are unchanged
    a, b = cases[3]
    sv, si = hip_ctx.segment_pair_energy(dv, None, a, b)
    assert np.array_equal(sv, hip_ctx.segment_pair_energy(dv, di, a, b)[0]) and np.all(si == 0.0)
    with pytest.raises(ValueError):
        hip_ctx.segment_pair_energy(dv, di, [0], [n + 1])


# ---- mode parity with the fixture's seeded stems -------------------------------------------------------------------
class _SeededStems:
    """Stands where the separator stands: returns the case's stems, resident on the device like the network's."""

    def __init__(self, hip, vocal, inst):
        self._primary_backend = types.SimpleNamespace(hip=hip)
        self.hip, self.vocal, self.inst, self.calls = hip, vocal, inst, 0

    def separate_for_detection(self, audio, *, gpu_context=None, audio_dev=None, **_):
        from audio_cut_amd.core.enhanced_vocal_separator import SeparationResult
        self.calls += 1
        hip = self.hip
        extra = {}
        state = {"hip": hip, "vocal": hip.to_device(self.vocal), "instrumental": hip.to_device(self.inst)}
        if np.ndim(audio) == 2:             # as the separator does: the mono mix (L + R) * 0.5, and [2, N] stems beside the mono ones
            state["mix_stereo"] = hip.to_device(audio)
            audio = (audio[0] + audio[1]) * np.float32(0.5)
            extra = {"mono_mix": audio, "vocal_track_stereo": np.stack([self.vocal, self.vocal]),
                     "instrumental_track_stereo": np.stack([self.inst, self.inst])}
        state["mix"] = hip.to_device(audio)
        return SeparationResult(vocal_track=self.vocal, instrumental_track=self.inst, separation_confidence=1.0, backend_used="seeded",
                                processing_time=0.0, quality_metrics={}, device_state=state, **extra)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "librosa_onset.npz")


def _golden_cases(golden):
    return json.loads(str(golden["cases"]))


def _split(hip, case):
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    mix, vocal, inst = onset_cases.build(case)
    stub = _SeededStems(hip, vocal, inst)
    saved = cfg.snapshot()
    cfg.set_runtime_config(dict(case["overrides"]))
    try:
        return SeamlessSplitter(SR, separator=stub).split_track(mix, mode="librosa_onset"), stub, (mix, vocal, inst)
    finally:
        cfg.restore(saved)


@pytest.mark.parametrize("name", [c["name"] for c in onset_cases.CASES])
def test_split_track_matches_the_reference(hip_ctx, golden, name):
    case = {c["name"]: c for c in _golden_cases(golden)}[name]
    res, stub, (mix, _, _) = _split(hip_ctx, case)
    assert res["mode"] == "librosa_onset" and res["method"] == "smart_segment_v2"
    if not case["success"]:
        assert res["success"] is False and "division by zero" in res["error"] and "cuts_samples" not in res
        return
    assert res["success"] is True
    bpm, bar_duration = (float(v) for v in golden[f"{name}__scalars"])
    assert res["bpm"] == bpm and res["bar_duration_s"] == bar_duration and res["density"] == case["density"]
    energies = golden[f"{name}__bar_energies"]
    got = np.asarray(res["bar_energies"], dtype=np.float64)
    assert got.shape == energies.shape
    worst = float(np.max(np.abs(got - energies) / energies))
    print(f"{name}: bpm {res['bpm']!r}, {len(got)} bars, worst bar-energy relative error {worst:.3e}")
    assert worst <= 1e-4
    assert res["bar_types"] == [TYPE_NAME[int(c)] for c in golden[f"{name}__bar_types"]]
    assert res["silence_boundaries"] == [float(s) for s in golden[f"{name}__silence_boundaries"]]
    cuts = [int(c) for c in golden[f"{name}__cuts"]]
    assert res["cuts_samples"] == cuts and res["sample_boundaries"] == cuts and cuts[-1] == len(mix)
    assert res["segment_vocal_flags"] == [bool(f) for f in golden[f"{name}__flags"]]
    use_vocal = case["overrides"].get("librosa_onset.use_vocal_separation", True)
    assert res["use_vocal_preprocessing"] is use_vocal and stub.calls == (1 if use_vocal else 0)
    if not use_vocal:                                                   # no separation: every segment is human, no stems come back
        assert all(res["segment_vocal_flags"]) and res["vocal_track"] is None and "vocal" not in res["device_state"]
    assert set(res["timings"]) == {"separate_s", "detect_s", "finalize_s"}


def test_split_track_stereo_detects_on_the_channel_mean(hip_ctx, golden):
    """A (2, N) track is split on its channel mean: the result of the mono track of those samples (no separation here, so no
    network run), and the stereo mix stays resident for the export."""
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    case = {c["name"]: c for c in _golden_cases(golden)}["c2_60s_no_separation"]
    mix, vocal, inst = onset_cases.build(case)
    side = (0.125 * np.sin(np.arange(len(mix)) * 0.01)).astype(np.float32)
    stereo = np.stack([mix + side, mix - side]).astype(np.float32)
    mean = (stereo[0] + stereo[1]) * np.float32(0.5)
    saved = cfg.snapshot()
    cfg.set_runtime_config(dict(case["overrides"]))
    try:
        splitter = SeamlessSplitter(SR, separator=_SeededStems(hip_ctx, vocal, inst))
        st = splitter.split_track(stereo, mode="librosa_onset")
        mono = splitter.split_track(mean, mode="librosa_onset")
    finally:
        cfg.restore(saved)
    assert st["success"] and st["cuts_samples"] == mono["cuts_samples"] and st["bpm"] == mono["bpm"]
    assert st["bar_energies"] == mono["bar_energies"]
    assert tuple(st["device_state"]["mix_stereo"].shape) == (2, len(mix))


def test_split_track_stereo_with_separation_keeps_the_stereo_stems(hip_ctx, golden):
    """The separation branch on a (2, N) track: cuts, bar analysis and labels of the mono track of its channel mean, with the
    mono mix and the [2, N] stems handed on for a two-channel export."""
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    case = {c["name"]: c for c in _golden_cases(golden)}["c2_60s_low"]
    mix, vocal, inst = onset_cases.build(case)
    side = (0.125 * np.sin(np.arange(len(mix)) * 0.01)).astype(np.float32)
    stereo = np.stack([mix + side, mix - side]).astype(np.float32)
    mean = (stereo[0] + stereo[1]) * np.float32(0.5)
    stub = _SeededStems(hip_ctx, vocal, inst)
    splitter = SeamlessSplitter(SR, separator=stub)
    st = splitter.split_track(stereo, mode="librosa_onset")
    mono = splitter.split_track(mean, mode="librosa_onset")
    assert stub.calls == 2 and st["success"] and st["use_vocal_preprocessing"] is True
    for key in ("bpm", "bar_energies", "bar_types", "silence_boundaries", "cuts_samples", "segment_vocal_flags", "segment_spans"):
        assert st[key] == mono[key], key
    assert set(st["segment_vocal_flags"]) == {True, False}
    assert np.array_equal(st["mono_mix"], mean) and "mono_mix" not in mono
    assert st["vocal_track_stereo"].shape == st["instrumental_track_stereo"].shape == (2, len(mix))
    assert tuple(st["device_state"]["mix_stereo"].shape) == (2, len(mix)) and st["device_state"]["mix"].dim() == 1


# ---- end to end with the real separator -----------------------------------------------------------------------------
def test_separate_and_segment_librosa_onset_end_to_end(hip_ctx, golden, tmp_path):
    from audio_cut_amd import api
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    case = {c["name"]: c for c in _golden_cases(golden)}["c2_60s_low"]
    mix, _, _ = onset_cases.build(case)
    src = tmp_path / "song.npy"
    np.save(src, mix)
    out_dir = tmp_path / "out"
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(out_dir), mode="librosa_onset", export_manifest=True)
    res = api.last_result()
    cuts = [int(c) for c in golden["c2_60s_low__cuts"]]
    assert res["cut_points_samples"] == cuts and man["cuts"]["samples"] == cuts          # the cuts do not depend on the stems
    assert man["version"] == "librosa_onset" and man["success"] is True and res["method"] == "smart_segment_v2"
    bpm, bar_duration = (float(v) for v in golden["c2_60s_low__scalars"])
    assert man["smart_segmentation"] == {"method": "smart_segment_v2", "bpm": bpm, "bar_duration_s": bar_duration, "density": "low",
                                         "silence_boundaries": [float(s) for s in golden["c2_60s_low__silence_boundaries"]]}
    assert man["export_plan"] == ["mix_segments"] and set(man["artifacts"]) == {"music_segments", "all", "output_dir"}
    files = sorted(p.relative_to(out_dir).as_posix() for p in out_dir.rglob("*") if p.is_file())
    assert len(files) == len(cuts) and "SegmentManifest.json" in files               # the mix segments and the manifest, nothing else
    assert all(f.startswith("segment_") and f.endswith(".wav") and "/" not in f for f in files if f != "SegmentManifest.json")
    assert len(man["segments"]) == len(cuts) - 1 == len(res["mix_segment_files"]) and not res["vocal_segment_files"]
    assert res["full_vocal_file"] is None and res["full_instrumental_file"] is None
    json.loads((out_dir / "SegmentManifest.json").read_text())

    # the labels against a float64 recomputation from the stems the product returns (the separation is deterministic: the
    # splitter run below returns the stems the call above labelled)
    direct = SeamlessSplitter(SR).split_track(mix, mode="librosa_onset")
    assert direct["cuts_samples"] == cuts and direct["segment_vocal_flags"] == res["segment_vocal_flags"]
    vocal, inst = direct["vocal_track"].astype(np.float64), direct["instrumental_track"].astype(np.float64)
    skipped = 0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        v, thr = float(np.sqrt(np.mean(vocal[a:b] ** 2))), 0.3 * float(np.sqrt(np.mean(inst[a:b] ** 2)))
        margin = abs(v - thr) / thr
        print(f"segment {i}: vocal_rms {v:.6e}  0.3 inst_rms {thr:.6e}  margin {margin:.3e}  label {res['segment_vocal_flags'][i]}")
        if margin < 1e-3:
            skipped += 1
            continue
        assert res["segment_vocal_flags"][i] == (v > thr), i
    assert skipped * 10 <= len(cuts) - 1, f"{skipped} of {len(cuts) - 1} segments too close to the threshold to check"

    # the vocal segments are honoured, the full stems are not written in this mode
    out2 = tmp_path / "out2"
    man2 = api.separate_and_segment(input_uri=str(src), export_dir=str(out2), mode="librosa_onset",
                                    export_types=["mix_segments", "vocal_segments", "full_vocal", "full_instrumental"])
    assert man2["export_plan"] == ["mix_segments", "vocal_segments"]
    assert set(man2["artifacts"]) == {"music_segments", "human_segments", "all", "output_dir"}
    assert len(list((out2 / "segments_vocal").glob("*_vocal_*.wav"))) == len(cuts) - 1
    assert not list(out2.glob("*vocal_full*")) and not list(out2.glob("*instrumental*"))


def test_separate_and_segment_reports_failure_without_writing_segments(hip_ctx, golden, tmp_path):
    from audio_cut_amd import api
    case = {c["name"]: c for c in _golden_cases(golden)}["c1_60s_fail"]
    mix, _, _ = onset_cases.build(case)
    src = tmp_path / "sine.npy"
    np.save(src, mix)
    out_dir = tmp_path / "out"
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(out_dir), mode="librosa_onset",
                                   runtime_overrides={"librosa_onset.use_vocal_separation": False})
    assert man["success"] is False and man["segments"] == [] and "smart_segmentation" not in man
    assert api.last_result()["success"] is False and "division by zero" in api.last_result()["error"]
    assert not [p for p in out_dir.rglob("*") if p.is_file()]


def test_separate_and_segment_librosa_onset_exports_both_channels(hip_ctx, golden, tmp_path):
    """`audio.channels: 2`: the real separator on true L/R, cuts from the channel mean, every WAV written with two channels."""
    import wave
    from audio_cut_amd import api
    case = {c["name"]: c for c in _golden_cases(golden)}["c2_60s_low"]
    mix, _, _ = onset_cases.build(case)
    side = (0.125 * np.sin(np.arange(len(mix)) * 0.01)).astype(np.float32)
    stereo = np.stack([mix + side, mix - side]).astype(np.float32)
    src = tmp_path / "song_stereo.npy"
    np.save(src, stereo)
    out_dir = tmp_path / "out"
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(out_dir), mode="librosa_onset",
                                   export_types=["mix_segments", "vocal_segments"], runtime_overrides={"audio.channels": 2})
    res = api.last_result()
    cuts = res["cut_points_samples"]
    assert man["success"] is True and man["audio"]["channels"] == 2 and man["smart_segmentation"]["method"] == "smart_segment_v2"
    assert cuts[0] == 0 and cuts[-1] == len(mix) and len(cuts) > 2
    assert len(res["mix_segment_files"]) == len(res["vocal_segment_files"]) == len(cuts) - 1
    for files in (res["mix_segment_files"], res["vocal_segment_files"]):
        total = 0
        for f in files:
            with wave.open(f, "rb") as w:
                assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 3, SR)
                total += w.getnframes()
        assert total == len(mix)                                              # the segments tile the track
    # the first mix segment holds L and R as they came in (PCM_24: within one quantisation step)
    with wave.open(res["mix_segment_files"][0], "rb") as w:
        raw = np.frombuffer(w.readframes(1000), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
    v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    v = np.where(v & 0x800000, v - 0x1000000, v).reshape(-1, 2) / 8388608.0
    assert np.max(np.abs(v - stereo[:, :1000].T)) <= 2.0 ** -23
