"""Segment finishing on the GPU: `acf_pack_spans` byte for byte against `pcm_bytes_host(finish_host(...))`, `acf_span_stats`
against `math.fsum`, the wrappers' refusals, both wrappers under poisoned allocations, and the three `quality_control` keys end to
end (include/finish/audiocut_finish.h, audio_cut_amd/_finish_native.py, audio_cut_amd/utils/segment_finish.py).

The span sets put a span boundary at every position of a group of four words, spans shorter than a group, more spans than a
workgroup has frames, gaps at both ends and between spans, and fade zones and boundaries across the first frame of a workgroup
(1024 words: frame 1024 k of a mono track, 512 k of a stereo one).

Infinities stand only where a fade weight is not zero: inf * 0 makes a NEW NaN, whose sign and payload IEEE 754 leaves open (a host and a
device need not agree on them), and the FLOAT and DOUBLE files keep NaN bits.  NaNs that come in are propagated, bits kept."""
import math
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import poison_alloc as PA
from audio_cut_amd.testing import signals
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import segment_finish as SF
from audio_cut_amd.utils import wav_reader as WR

pytestmark = pytest.mark.gpu

SR = 44100
SUBTYPES = ("PCM_U8", "PCM_16", "PCM_24", "PCM_32", "FLOAT", "DOUBLE")
WIDTH = {"PCM_U8": 1, "PCM_16": 2, "PCM_24": 3, "PCM_32": 4, "FLOAT": 4, "DOUBLE": 8}
FRAMES = (3, 5, 1023, 1025, 4099, 65539)
FADES = ((0, 0), (1, 1), (2, 0), (0, 2), (441, 882), (700, 700))
GAINS = np.array([1.0, 0.37, 3.0, 10.0], dtype=np.float32)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def kernels(hip_ctx):
    from audio_cut_amd._finish_native import FinishKernels
    return FinishKernels(hip_ctx)


# ---- span sets ------------------------------------------------------------------------------------------------------------------
def _walk(n, lengths, gaps, start):
    """Spans of the cycled `lengths` separated by the cycled `gaps`, from `start` on, as many as fit in front of frame n - 1."""
    spans, pos, k = [], start, 0
    while True:
        length = lengths[k % len(lengths)]
        if pos + length > n - 1:
            return spans
        spans.append((pos, pos + length))
        pos += length + gaps[k % len(gaps)]
        k += 1


def span_sets(n, fi, fo):
    sets = {"whole": [(0, n)]}
    lengths = [v for v in (1, 2, 3, fi, fi + 1, fi + fo - 1) if v > 0]
    residues = _walk(n, lengths, gaps=(1, 0, 2, 3, 0, 1, 5), start=1)
    if residues:
        sets["residues"] = residues
        if n >= 4099:
            assert {a % 4 for a, _ in residues} == {b % 4 for _, b in residues} == {0, 1, 2, 3}
            assert any(b < c for (_, b), (c, _) in zip(residues, residues[1:])) and residues[-1][1] < n
    rng = np.random.default_rng(n)
    dense = _walk(n, [int(v) for v in rng.integers(1, 8, 300)], gaps=[int(v) for v in rng.integers(0, 3, 300)], start=2)[:300]
    if n >= 4099:
        assert len(dense) == 300 and dense[-1][1] < 2048           # more spans than a workgroup has frames
    if dense:
        sets["dense"] = dense
    if n >= 4099:
        # the fade-in zone lies across frame 1024, the fade-out zone across frame 2048, a boundary on frame 3072
        a, b = 1024 - (fi + 1) // 2, 2048 + (fo + 1) // 2
        sets["across"] = [(a, b), (b + 3, 3072), (3072, min(n, 4096 + 3))]
        assert (fi < 2 or a < 1024 < a + fi) and (fo < 2 or b - fo < 2048 < b)
    if (fi, fo) == (700, 700) and n >= 1023:
        sets["both_fades"] = [(13, 1013)]                           # Fi + Fo > L: 400 frames take both weights
    return sets


def _gains(k):
    return GAINS[(np.arange(k) * 3 + 1) % 4]


def _input(n, channels, spans):
    """Planar [channels, n] noise of scale 0.6 with NaN, -0.0 and a denormal in a fade zone (the second frame of a span, the frame
    before its last) and in its interior, on alternating channels, and the infinities at frames whose weights are not zero."""
    rng = np.random.default_rng(100 * n + channels)
    x = (0.6 * rng.standard_normal((channels, n))).astype(np.float32)
    specials = np.array([np.nan, -0.0, 1e-45, np.inf, -np.inf], dtype=np.float32)
    placed = 0
    for lo, hi in spans:
        if hi - lo >= 12 and placed < 6:
            for j, at in enumerate((lo + 1, lo + 2, lo + 3, lo + 4, lo + 5, hi - 2, hi - 3, hi - 4, hi - 5, hi - 6,
                                    lo + (hi - lo) // 2, lo + (hi - lo) // 2 + 1)):
                x[(j + placed) % channels, at] = specials[j % 5]
            placed += 1
    if n >= 3:
        x[0, 1] = np.nan if not placed else x[0, 1]
    return x


_HOST = {}


def _host_case(n, channels, fi, fo, name, spans):
    """(input, finished float32 track) of a case: computed once, shared by the six subtypes."""
    key = (n, channels, fi, fo, name)
    if key not in _HOST:
        x = _input(n, channels, spans)
        y = SF.finish_host(x if channels == 2 else x[0], spans, _gains(len(spans)), fi, fo)
        x.setflags(write=False); y.setflags(write=False)
        _HOST[key] = (x, y)
    return _HOST[key]


def _upload(hip, x, channels):
    """The shared (read-only) planar input as a device track: [2, n], or [n] for one channel."""
    return hip.to_device(np.array(x if channels == 2 else x[0]))


def _pack_checked(kernels, xd, spans, gains, fi, fo, subtype):
    """pack_spans_device into a buffer with 16 sentinel bytes behind the sample bytes, which must survive."""
    n_bytes = int(xd.shape[-1]) * xd.dim() * WIDTH[subtype]
    out = torch.full((n_bytes + 16,), SENTINEL, dtype=torch.uint8, device=kernels.device)
    got = kernels.pack_spans_device(xd, spans, gains, fi, fo, subtype, out=out)
    assert got.numel() == n_bytes and got.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    assert (host[n_bytes:] == SENTINEL).all(), f"{subtype}: bytes behind the output were written"
    return host[:n_bytes]


def _first_difference(got, want, width, channels):
    at = int(np.flatnonzero(got != want)[0])
    return f"first differing byte {at} = word {at // width} = frame {at // (width * channels)}"


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("subtype", SUBTYPES)
def test_pack_spans_is_the_host_statement(hip_ctx, kernels, subtype, channels):
    for n in FRAMES:
        for fi, fo in FADES:
            for name, spans in span_sets(n, fi, fo).items():
                x, y = _host_case(n, channels, fi, fo, name, spans)
                want, width = AE.pcm_bytes_host(y.T if channels == 2 else y, subtype)
                xd = _upload(hip_ctx, x, channels)
                got = _pack_checked(kernels, xd, spans, _gains(len(spans)), fi, fo, subtype)
                assert got.tobytes() == want.tobytes(), (subtype, channels, n, fi, fo, name, _first_difference(got, want, width, channels))
    # the finished track is not the plain one (the check above is not vacuous), and the wrapper that downloads gives the same bytes
    spans = span_sets(4099, 441, 882)["across"]
    x, y = _host_case(4099, channels, 441, 882, "across", spans)
    xd = _upload(hip_ctx, x, channels)
    want, _ = AE.pcm_bytes_host(y.T if channels == 2 else y, subtype)
    assert kernels.pack_spans(xd, spans, _gains(len(spans)), 441, 882, subtype).tobytes() == want.tobytes()
    assert want.tobytes() != hip_ctx.pack_pcm(xd, subtype).tobytes()


@pytest.mark.parametrize("subtype", SUBTYPES)
def test_pack_spans_rows_and_alignment(hip_ctx, kernels, subtype):
    """Stereo rows that stand in wider rows at an even stride (the 8-byte loads) and an odd one (sample by sample), a stereo track
    that starts at an odd sample, and a mono track that is not 16-byte aligned: all converted, the gap between the rows not read."""
    fi, fo = 441, 882
    for n, stride, offset in ((4099, 4104, 0), (4099, 4103, 0), (1025, 1032, 1), (5, 6, 0)):
        for name, spans in span_sets(n, fi, fo).items():
            x, y = _host_case(n, 2, fi, fo, name, spans)
            base = torch.full((2, stride + offset), 7.0, dtype=torch.float32, device=hip_ctx.device)
            base[:, offset: offset + n] = _upload(hip_ctx, x, 2)
            xd = base[:, offset: offset + n]
            assert xd.stride(0) == stride + offset and not xd.is_contiguous()
            want, _ = AE.pcm_bytes_host(y.T, subtype)
            assert _pack_checked(kernels, xd, spans, _gains(len(spans)), fi, fo, subtype).tobytes() == want.tobytes(), (n, stride, offset, name)
    for n, offset in ((4099, 1), (1023, 3), (5, 2)):
        for name, spans in span_sets(n, fi, fo).items():
            x, y = _host_case(n, 1, fi, fo, name, spans)
            base = torch.zeros(n + offset, dtype=torch.float32, device=hip_ctx.device)
            base[offset:] = _upload(hip_ctx, x, 1)
            assert base[offset:].data_ptr() % 16 != 0
            want, _ = AE.pcm_bytes_host(y, subtype)
            assert _pack_checked(kernels, base[offset:], spans, _gains(len(spans)), fi, fo, subtype).tobytes() == want.tobytes(), (n, offset, name)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("subtype", SUBTYPES)
def test_pack_spans_with_nothing_to_do_is_pack_pcm(hip_ctx, kernels, subtype, channels):
    for n in FRAMES:
        for name, spans in span_sets(n, 0, 0).items():
            x, _ = _host_case(n, channels, 0, 0, name, spans)
            xd = _upload(hip_ctx, x, channels)
            got = _pack_checked(kernels, xd, spans, np.ones(len(spans), dtype=np.float32), 0, 0, subtype)
            assert got.tobytes() == hip_ctx.pack_pcm(xd, subtype).tobytes(), (subtype, channels, n, name)


# ---- acf_span_stats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_span_stats_against_fsum(hip_ctx, kernels, channels):
    for n in FRAMES:
        for fi, fo in FADES:
            for name, spans in span_sets(n, fi, fo).items():
                rng = np.random.default_rng(7 * n + channels)
                x = (0.6 * rng.standard_normal((channels, n))).astype(np.float32)
                silent = len(spans) // 2 if len(spans) > 1 else None
                if silent is not None:                                              # a silent span
                    x[:, spans[silent][0]: spans[silent][1]] = 0.0
                track = x if channels == 2 else x[0]
                xd = hip_ctx.to_device(track)
                sumsq, peak = kernels.span_stats(xd, spans, fi, fo)
                assert sumsq.dtype == np.float64 and peak.dtype == np.float32 and sumsq.shape == peak.shape == (len(spans),)
                faded = SF.finish_host(track, spans, np.ones(len(spans), dtype=np.float32), fi, fo).reshape(channels, n)
                for k, (a, b) in enumerate(spans):
                    seg = faded[:, a:b]
                    want = math.fsum((seg.astype(np.float64) ** 2).reshape(-1).tolist())
                    assert peak[k] == np.abs(seg).max(), (n, fi, fo, name, k)
                    assert abs(sumsq[k] - want) <= (b - a) * channels * 2.0 ** -53 * want, (n, fi, fo, name, k, sumsq[k], want)
                assert silent is None or (sumsq[silent] == 0.0 and peak[silent] == 0.0)
                again = kernels.span_stats(xd, spans, fi, fo)
                assert again[0].tobytes() == sumsq.tobytes() and again[1].tobytes() == peak.tobytes()
    # the host's own statement agrees to the same bound
    spans = span_sets(4099, 441, 882)["across"]
    x = (0.6 * np.random.default_rng(3).standard_normal((channels, 4099))).astype(np.float32)
    track = x if channels == 2 else x[0]
    got, pk = kernels.span_stats(hip_ctx.to_device(track), spans, 441, 882)
    want, want_pk = SF.finish_stats_host(track, spans, 441, 882)
    assert pk.tobytes() == want_pk.tobytes() and np.all(np.abs(got - want) <= 4099 * channels * 2.0 ** -53 * want)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
def test_wrapper_refusals(hip_ctx, kernels):
    from audio_cut_amd import _native
    dev = hip_ctx.device
    x = torch.zeros(64, device=dev)
    one = np.ones(1, dtype=np.float32)
    for spans in ([(10, 20), (0, 5)], [(0, 10), (9, 20)], [(5, 5)], [(7, 3)], [(0, 65)], [(-1, 4)], [], [(1, 2, 3)]):
        g = np.ones(len(spans), dtype=np.float32)
        with pytest.raises(ValueError, match="span"):
            kernels.pack_spans(x, spans, g, 0, 0, "FLOAT")
        with pytest.raises(ValueError, match="span"):
            kernels.span_stats(x, spans, 0, 0)
    for bad in (torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros((3, 64), device=dev), torch.zeros(0, device=dev),
                torch.zeros(128, device=dev)[::2], torch.zeros((2, 2, 2), device=dev), torch.zeros(64), np.zeros(64, np.float32)):
        with pytest.raises(_native.NativeError):
            kernels.pack_spans(bad, [(0, 1)], one, 0, 0, "PCM_16")
        with pytest.raises(_native.NativeError):
            kernels.span_stats(bad, [(0, 1)], 0, 0)
    with pytest.raises(ValueError, match="ULAW"):
        kernels.pack_spans(x, [(0, 64)], one, 0, 0, "ULAW")
    for gains in (np.ones(1, dtype=np.float64), np.ones(2, dtype=np.float32), [1.0]):
        with pytest.raises(ValueError, match="gains"):
            kernels.pack_spans(x, [(0, 64)], gains, 0, 0, "FLOAT")
    for fades in ((-1, 0), (0, -1), (1.5, 0)):
        with pytest.raises(ValueError, match="fades"):
            kernels.pack_spans(x, [(0, 64)], one, *fades, "FLOAT")
        with pytest.raises(ValueError, match="fades"):
            kernels.span_stats(x, [(0, 64)], *fades)
    with pytest.raises(_native.NativeError):
        kernels.pack_spans_device(x, [(0, 64)], one, 0, 0, "PCM_32", out=torch.zeros(255, dtype=torch.uint8, device=dev))
    with pytest.raises(_native.NativeError, match="aligned"):            # the library's own check: a PCM_32 stream needs 16 bytes
        kernels.pack_spans_device(x, [(0, 64)], one, 0, 0, "PCM_32", out=torch.zeros(512, dtype=torch.uint8, device=dev)[4:])
    # and what is not refused still works afterwards
    assert kernels.pack_spans(x, [(0, 64)], one, 0, 0, "PCM_16").tobytes() == bytes(128)


def test_finish_wrappers_under_poison(hip_ctx, kernels):
    """Every output byte is written, nothing outside is touched and no read outside the inputs reaches a result: unpoisoned, under
    0xFF and under 0x7F the results are the same bits and every guard band is intact."""
    for channels, n, fi, fo, name in ((1, 4099, 441, 882, "across"), (2, 4099, 441, 882, "residues"), (2, 1025, 2, 0, "dense"),
                                      (1, 5, 1, 1, "whole"), (2, 3, 0, 2, "whole")):
        spans = span_sets(n, fi, fo)[name]
        x, y = _host_case(n, channels, fi, fo, name, spans)
        finite = np.nan_to_num(x, nan=0.25, posinf=0.5, neginf=-0.5)
        gains = _gains(len(spans))

        def run(upload):
            xd = upload(np.array(x if channels == 2 else x[0]))
            fd = upload(finite if channels == 2 else finite[0])
            return {"stats": kernels.span_stats(fd, spans, fi, fo),
                    "bytes": {st: kernels.pack_spans(xd, spans, gains, fi, fo, st) for st in SUBTYPES}}

        clean = PA.run_three(hip_ctx, run)
        for st in SUBTYPES:
            assert clean["bytes"][st].tobytes() == AE.pcm_bytes_host(y.T if channels == 2 else y, st)[0].tobytes()
        assert np.isfinite(clean["stats"][0]).all() and np.isfinite(clean["stats"][1]).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
SONG_SECONDS, SONG_SEED = 30.0, 12
ON = {"quality_control.fade_in_duration": 0.01, "quality_control.fade_out_duration": 0.02, "quality_control.normalize_audio": True}


def _write_wav(path, x):
    """16-bit PCM, mono [n] or planar [2, n]."""
    pcm = np.clip(np.rint(np.atleast_2d(x).T * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1]); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())


def _data(path):
    """(WavInfo, float32 [n_frames, channels]) of a file."""
    info = WR.read_wav_info(path)
    return info, np.asarray(WR.decode_samples(WR.read_wav_bytes(path, info), info), dtype=np.float32).reshape(info.n_frames, info.channels)


def _relative(paths, root):
    return [Path(p).relative_to(root).as_posix() for p in paths]


def test_finish_end_to_end(hip_ctx, tmp_path):
    from audio_cut_amd import api
    src = tmp_path / "song.wav"
    _write_wav(src, signals.c2_song(SONG_SECONDS, seed=SONG_SEED))
    runs = {}
    for key, over in (("a", {}), ("b", ON)):
        man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / key),
                                       runtime_overrides={"output.wav.subtype": "FLOAT", **over})
        res = api.last_result()
        assert res["success"] is True
        runs[key] = (res, man)
    (res_a, man_a), (res_b, man_b) = runs["a"], runs["b"]
    n_seg = res_a["num_segments"]
    assert n_seg >= 3 and len(res_a["mix_segment_files"]) == len(res_a["vocal_segment_files"]) == n_seg
    # the same cuts and names; the new keys only where finishing is on
    assert res_b["cut_points_samples"] == res_a["cut_points_samples"]
    assert _relative(res_b["saved_files"], tmp_path / "b") == _relative(res_a["saved_files"], tmp_path / "a")
    assert set(res_b) - set(res_a) == {"segment_finish"} and set(res_a) - set(res_b) == set()
    assert set(man_b) - set(man_a) == {"finish"} and set(man_a) - set(man_b) == set()
    # the full tracks stay plain
    for field in ("full_vocal_file", "full_instrumental_file"):
        assert res_a[field] and Path(res_b[field]).read_bytes() == Path(res_a[field]).read_bytes(), field
    block = man_b["finish"]
    assert block is res_b["segment_finish"] or block == res_b["segment_finish"]
    assert (block["fade_in_frames"], block["fade_out_frames"]) == (441, 882)
    assert block["settings"] == {"fade_in_duration": 0.01, "fade_out_duration": 0.02, "normalize_audio": True,
                                 "normalize_target_db": -20.0, "normalize_max_gain": 10.0}
    assert len(block["mix"]) == len(block["vocal"]) == n_seg
    settings = SF.finish_settings({k.split(".")[1]: v for k, v in ON.items()}, SR)
    changed = 0
    for kind, field in (("mix", "mix_segment_files"), ("vocal", "vocal_segment_files")):
        for i, (pa, pb) in enumerate(zip(res_a[field], res_b[field])):
            (info_a, xa), (info_b, xb) = _data(pa), _data(pb)
            assert info_b.sample_format == "f32" and (info_a.n_frames, info_a.channels) == (info_b.n_frames, info_b.channels) == (len(xa), 1)
            row = block[kind][i]
            assert set(row) == {"gain", "gain_db", "rms_db", "peak_out", "clipped"} and row["clipped"] is False
            gain = np.float32(row["gain"])
            assert float(gain) == row["gain"]
            length = len(xa)
            assert length > 882
            want = SF.finish_host(xa[:, 0], [(0, length)], np.array([gain]), 441, 882)
            assert xb[:, 0].tobytes() == want.tobytes(), f"{kind} segment {i} is not the finished segment of the plain run"
            faded = SF.finish_host(xa[:, 0], [(0, length)], np.ones(1, np.float32), 441, 882).astype(np.float64)
            sumsq = math.fsum((faded * faded).tolist())
            expect = SF.gain_from_stats(sumsq, length, settings)
            assert abs(float(gain) - float(expect)) <= float(np.spacing(expect)), (kind, i, gain, expect)
            if sumsq > 0.0:
                assert row["rms_db"] == pytest.approx(10.0 * math.log10(sumsq / length), abs=1e-9)
                assert row["gain_db"] == pytest.approx(20.0 * math.log10(float(gain)), abs=1e-12)
            assert xb[0, 0] == 0.0 and xb[-1, 0] == 0.0
            changed += int(xb.tobytes() != xa.tobytes())
    assert changed == 2 * n_seg
    # another export rate is refused by name before anything is loaded or written
    with pytest.raises(ValueError, match=r"quality_control\.normalize_audio.*output\.sample_rate"):
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "c"),
                                 runtime_overrides={"quality_control.normalize_audio": True, "output.sample_rate": 48000})
    assert not (tmp_path / "c").exists() or not any((tmp_path / "c").rglob("*"))


def test_finish_end_to_end_pcm16_stereo(hip_ctx, tmp_path):
    from audio_cut_amd import api
    src = tmp_path / "song.wav"
    _write_wav(src, signals.c2_song(SONG_SECONDS, seed=SONG_SEED, stereo=True))
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"),
                                   runtime_overrides={"audio.channels": 2, "output.wav.subtype": "PCM_16", **ON})
    res = api.last_result()
    assert res["success"] is True and man["audio"]["channels"] == 2
    cuts = res["cut_points_samples"]
    n_seg = res["num_segments"]
    assert n_seg >= 3 and len(man["finish"]["mix"]) == len(man["finish"]["vocal"]) == n_seg
    lengths = [int(round(d * SR)) for d in res["segment_durations"]]
    assert len(lengths) == n_seg and min(lengths) > 882 and len(cuts) >= 2
    for field in ("mix_segment_files", "vocal_segment_files"):
        assert len(res[field]) == n_seg
        for path, length in zip(res[field], lengths):
            info, x = _data(path)
            assert (info.sample_format, info.channels, info.n_frames, info.sample_rate) == ("s16", 2, length, SR), path
            # Fi = 441 > 1 and Fo = 882 > 1: the first and the last frame carry the weight 0 on both channels, and a frame inside
            # the fade-in carries ONE weight: the channels keep their ratio where the plain track has it
            assert x[0].tolist() == [0.0, 0.0] and x[-1].tolist() == [0.0, 0.0], path
    # the full tracks are the plain conversion of a run without the keys
    api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "plain"),
                             runtime_overrides={"audio.channels": 2, "output.wav.subtype": "PCM_16"})
    plain = api.last_result()
    assert "segment_finish" not in plain
    for field in ("full_vocal_file", "full_instrumental_file"):
        assert Path(res[field]).read_bytes() == Path(plain[field]).read_bytes(), field
    # both channels of a frame carry the same weight: frame i of a fade-in is the plain frame times w[i] * gain on either channel.
    # A decoded 16-bit word is at most 2^-15 below its float sample (the word is a floor), on either side of the comparison, the
    # plain side scaled by w * g <= g; the float32 roundings in between are 2^-24 relative.  Frames that would clip are left out.
    w = np.linspace(0, 1, 441)
    compared = 0
    for path_b, path_a, row in zip(res["mix_segment_files"], plain["mix_segment_files"], man["finish"]["mix"]):
        (_, xb), (_, xa) = _data(path_b), _data(path_a)
        g = float(np.float32(row["gain"]))
        for i in (1, 100, 440):
            for c in (0, 1):
                if abs(xa[i, c]) * w[i] * g < 0.99:
                    assert abs(xb[i, c] - xa[i, c] * w[i] * g) <= (1.0 + g) * 2.0 ** -15 + 1e-6, (path_b, i, c)
                    compared += 1
    assert compared >= 3 * n_seg
