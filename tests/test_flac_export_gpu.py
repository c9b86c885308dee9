"""FLAC export on the GPU: `FlacKernels.encode` byte for byte against the host statement `flac_encode_host`, every device stream
through the independent decoder of tests/flac_decode.py, both launches under the poisoned, guarded allocator, the wrapper's
refusals, and `separate_and_segment` with `output.format: flac` end to end against a second run with `wav`."""
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import poison_alloc as PA
from flac_decode import flac_decode
from flac_signals import COUNTS, SR, signals
from audio_cut_amd.testing import signals as track_signals
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import flac_export as FX

pytestmark = pytest.mark.gpu

SUBTYPES = (("PCM_16", 2), ("PCM_24", 3))


@pytest.fixture(scope="module")
def kernels(hip_ctx):
    from audio_cut_amd._flac_native import FlacKernels
    return FlacKernels(hip_ctx)


def _grid_track(channels: int):
    """Every signal at every count, one behind the other: (float32 [n, channels], spans, names)."""
    parts, spans, names, at = [], [], [], 0
    for n in COUNTS:
        for name, x in signals(n, channels):
            parts.append(x.reshape(n, channels))
            spans.append((at, at + n))
            names.append(f"{name}[{n}]")
            at += n
    return np.concatenate(parts), spans, names


def _first_difference(got: bytes, want: bytes) -> str:
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


def _check(kernels, hip, pcm, n, channels, width, rate, spans, block_size, names=None, md5=False):
    """Device files == host files, byte for byte; every device file decodes to its span of the PCM words."""
    got = kernels.encode(torch.from_numpy(np.array(pcm)).to(hip.device), n, channels, width, rate, spans, block_size, md5=md5)
    want = FX.flac_encode_host(pcm, n, channels, width, rate, spans, block_size, md5=md5)
    words = FX.pcm_words(pcm, n, channels, width)
    assert len(got) == len(want) == len(spans)
    for i, ((lo, hi), g, w) in enumerate(zip(spans, got, want)):
        label = names[i] if names else f"span {i} [{lo}, {hi})"
        assert g == w, f"{label}: {_first_difference(g, w)}"
        decoded, info = flac_decode(g)
        assert decoded.shape == (hi - lo, channels) and (decoded == words[lo:hi]).all(), label
        assert (info["sample_rate"], info["bits"], info["min_block"]) == (rate, 8 * width, block_size)
    return got


@pytest.mark.parametrize("block_size", (256, 4096))
@pytest.mark.parametrize("subtype,width", SUBTYPES)
@pytest.mark.parametrize("channels", (1, 2))
def test_device_bytes_equal_the_host_statement(hip_ctx, kernels, channels, subtype, width, block_size):
    track, spans, names = _grid_track(channels)
    pcm, w = AE.pcm_bytes_host(track.reshape(-1), subtype)
    assert w == width
    _check(kernels, hip_ctx, pcm, track.shape[0], channels, width, SR, spans, block_size, names)


@pytest.mark.parametrize("frames", (130, 2050))
def test_frame_number_code_boundaries(hip_ctx, kernels, frames):
    """Silence at block 256 and 16 bits: the frame number's code grows to two bytes at 128 and to three at 2048."""
    n = 256 * frames
    pcm = np.zeros(2 * n, dtype=np.uint8)
    (got,) = kernels.encode(torch.from_numpy(pcm).to(hip_ctx.device), n, 1, 2, SR, [(0, n)], 256)
    (want,) = FX.flac_encode_host(pcm, n, 1, 2, SR, [(0, n)], 256)
    assert got == want, _first_difference(got, want)
    decoded, info = flac_decode(got)
    assert decoded.shape == (n, 1) and not decoded.any() and info["frames"] == frames


def _residue_spans(n: int):
    """Spans whose first and last PCM byte fall on every residue modulo 4, that overlap, and spans of 1 and 2 samples."""
    spans = [(lo, n - hi) for lo in range(4) for hi in range(4)]                 # nested: every pair overlaps
    spans += [(lo, lo + 1) for lo in (0, 1, 2, 3, n - 1)] + [(lo, lo + 2) for lo in (0, 1, 2, 3, n - 2)]
    spans += [(5, 5 + 257), (100, 100 + 4097), (7, 7 + 4096), (n // 2, n // 2 + 15)]
    return spans


@pytest.mark.parametrize("subtype,width", SUBTYPES)
@pytest.mark.parametrize("channels", (1, 2))
def test_spans_at_every_residue(hip_ctx, kernels, channels, subtype, width):
    n = 9001
    rng = np.random.default_rng(11)
    x = (0.4 * np.sin(np.arange(n)[:, None] / np.array([9.0, 13.0])[None, :channels]) + 0.02 * rng.standard_normal((n, channels))).astype(np.float32)
    pcm, _ = AE.pcm_bytes_host(x.reshape(-1), subtype)
    spans = _residue_spans(n)
    stride = channels * width
    reachable = {r * stride % 4 for r in range(4)}                                  # all four with 3-byte frames, two with 2 and 6
    assert {lo * stride % 4 for lo, _ in spans} == reachable == {hi * stride % 4 for _, hi in spans}
    got = _check(kernels, hip_ctx, pcm, n, channels, width, 48000, spans, 1024, md5=True)
    # where the frames land in the stream: the header's 42 bytes apart, the offsets are the running sum of the files before
    offsets = np.cumsum([0] + [len(g) - 42 for g in got])
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3}
    stream, files = kernels.encode_device(torch.from_numpy(np.array(pcm)).to(hip_ctx.device), n, channels, width, 48000, spans, 1024)
    assert [f[0] for f in files] == offsets[:-1].tolist() and stream.numel() == offsets[-1]
    for (off, length, smallest, largest), g in zip(files, got):
        assert stream[off: off + length].cpu().numpy().tobytes() == g[42:]
        assert int.from_bytes(g[12:15], "big") == smallest and int.from_bytes(g[15:18], "big") == largest


def test_wrapper_refusals(hip_ctx, kernels):
    dev = hip_ctx.device
    pcm = torch.zeros(600, dtype=torch.uint8, device=dev)
    ok = dict(pcm_dev=pcm, n_frames=100, channels=2, width=3, sample_rate=SR, spans=[(0, 100)], block_size=4096)
    for change, error in ((dict(width=4), ValueError), (dict(width=1), ValueError), (dict(channels=3), ValueError),
                          (dict(block_size=4000), ValueError), (dict(sample_rate=2_000_000), ValueError), (dict(spans=[]), ValueError),
                          (dict(spans=[(3, 3)]), ValueError), (dict(spans=[(0, 101)]), ValueError), (dict(spans=[(-1, 5)]), ValueError),
                          (dict(n_frames=0), ValueError), (dict(n_frames=99), Exception), (dict(pcm_dev=pcm.cpu()), Exception),
                          (dict(pcm_dev=pcm.to(torch.int8)), Exception), (dict(pcm_dev=torch.zeros(1200, dtype=torch.uint8, device=dev)[::2]), Exception)):
        with pytest.raises(error):
            kernels.encode_device(**{**ok, **change})
    # and what is not refused still works afterwards
    (data,) = kernels.encode(**ok)
    decoded, _ = flac_decode(data)
    assert decoded.shape == (100, 2) and not decoded.any()


def test_encoder_under_poison(hip_ctx, kernels):
    """Every byte of the stream, of the records and of the lengths is written, nothing outside is touched: unpoisoned, under 0xFF
    and under 0x7F the results are the same bits, and every guard band - the bytes behind the stream's end included - is intact."""
    for channels, (subtype, width), block_size, n in ((1, SUBTYPES[0], 256, 1301), (2, SUBTYPES[1], 4096, 9001), (2, SUBTYPES[0], 1024, 4099)):
        rng = np.random.default_rng(n)
        x = np.concatenate([0.5 * np.sin(np.arange(n - 700)[:, None] / np.array([5.0, 6.0])[None, :channels]),
                            np.zeros((300, channels)), rng.uniform(-0.9, 0.9, (400, channels))]).astype(np.float32)
        pcm, _ = AE.pcm_bytes_host(x.reshape(-1), subtype)
        spans = [(0, n), (3, n - 2), (n - 1, n), (1, 3), (n // 3, n // 3 + block_size + 1)]

        def run(upload):
            stream, files = kernels.encode_device(upload(np.array(pcm)), n, channels, width, SR, spans, block_size)
            return {"stream": stream, "files": files}

        clean = PA.run_three(hip_ctx, run)
        data = clean["stream"].cpu().numpy()
        want = FX.flac_encode_host(pcm, n, channels, width, SR, spans, block_size)
        for (off, length, _, _), w in zip(clean["files"], want):
            assert data[off: off + length].tobytes() == w[42:]
        assert sum(f[1] for f in clean["files"]) == data.size


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
SONG_SECONDS, SONG_SEED = 12.3, 4
FINISH_ON = {"quality_control.fade_in_duration": 0.01, "quality_control.fade_out_duration": 0.02, "quality_control.normalize_audio": True}


def _write_wav(path, x):
    """16-bit PCM, mono [n] or planar [2, n]."""
    pcm = np.clip(np.rint(np.atleast_2d(x).T * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1]); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())


def _wav_words(path):
    """(int64 [n, channels], rate) of an integer WAV of 44 header bytes as this build writes them."""
    raw = Path(path).read_bytes()
    assert raw[:4] == b"RIFF" and raw[36:40] == b"data"
    channels, rate, width = int.from_bytes(raw[22:24], "little"), int.from_bytes(raw[24:28], "little"), int.from_bytes(raw[34:36], "little") // 8
    size = int.from_bytes(raw[40:44], "little")
    return FX.pcm_words(raw[44: 44 + size], size // (channels * width), channels, width), rate, 8 * width


CASES = {
    "default": ("v2.2_mdd", False, {}, {}),
    "stereo_pcm16": ("v2.2_mdd", True, {"audio.channels": 2, "output.flac.subtype": "PCM_16", "output.flac.block_size": 1024},
                     {"audio.channels": 2, "output.wav.subtype": "PCM_16"}),
    "rate_48000": ("v2.2_mdd", False, {"output.sample_rate": 48000}, {"output.sample_rate": 48000}),
    "finished": ("v2.2_mdd", False, dict(FINISH_ON), dict(FINISH_ON)),
    "vocal_separation": ("vocal_separation", False, {"output.flac.md5": True}, {}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_end_to_end_against_the_wav_run(hip_ctx, tmp_path, case):
    from audio_cut_amd import api
    mode, stereo, flac_over, wav_over = CASES[case]
    src = tmp_path / "song.wav"
    _write_wav(src, track_signals.c2_song(SONG_SECONDS, seed=SONG_SEED, stereo=stereo))
    runs = {}
    for key, over in (("flac", {"output.format": "flac", **flac_over}), ("wav", {"output.format": "wav", **wav_over})):
        man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / key), mode=mode, runtime_overrides=over)
        res = api.last_result()
        assert res["success"] is True
        runs[key] = (res, man)
    (res_f, man_f), (res_w, man_w) = runs["flac"], runs["wav"]
    assert man_f["export_format"] == res_f["export_format"] == "flac"
    assert "export_format" not in man_w and "export_format" not in res_w
    assert set(res_f) - set(res_w) == {"export_format"} and set(man_f) - set(man_w) == {"export_format"}
    rel_f = [Path(p).relative_to(tmp_path / "flac") for p in res_f["saved_files"]]
    rel_w = [Path(p).relative_to(tmp_path / "wav") for p in res_w["saved_files"]]
    assert rel_f and len(rel_f) == len(rel_w) and len(set(rel_f)) == len(rel_f)
    if mode == "vocal_separation":
        assert len(rel_f) == 2
    else:
        assert res_f["cut_points_samples"] == res_w["cut_points_samples"]
        assert res_f["num_segments"] >= 2 and len(res_f["mix_segment_files"]) == len(res_f["vocal_segment_files"]) == res_f["num_segments"]
        assert res_f["full_vocal_file"] and res_f["full_instrumental_file"]
    block = int(flac_over.get("output.flac.block_size", 4096))
    pcm_bytes = flac_bytes = 0
    for a, b in zip(rel_f, rel_w):
        assert a.suffix == ".flac" and b.suffix == ".wav" and a.with_suffix("") == b.with_suffix(""), (a, b)
        data = (tmp_path / "flac" / a).read_bytes()
        got, info = flac_decode(data)
        want, rate, bits = _wav_words(tmp_path / "wav" / b)
        assert got.shape == want.shape and (got == want).all(), a
        assert (info["sample_rate"], info["bits"], info["channels"], info["min_block"]) == (rate, bits, 2 if stereo else 1, block)
        if flac_over.get("output.flac.md5"):
            import hashlib
            assert info["md5"] == hashlib.md5((tmp_path / "wav" / b).read_bytes()[44:]).digest()
        else:
            assert info["md5"] == bytes(16)
        pcm_bytes += want.size * bits // 8
        flac_bytes += len(data)
    print(f"{case}: {len(rel_f)} files, {flac_bytes} FLAC bytes for {pcm_bytes} PCM bytes ({flac_bytes / pcm_bytes:.3f})")


def test_a_run_without_the_key_is_the_wav_run_and_imports_nothing(hip_ctx, tmp_path):
    """With `output.format` absent: the files of a run with `wav`, byte for byte, whose mix segments are the input's own 16-bit
    words as PCM_24 (word << 8: nothing of that depends on this build's history), and neither FLAC module is imported."""
    from audio_cut_amd import api
    names = ("audio_cut_amd._flac_native", "audio_cut_amd.utils.flac_export")
    held = {name: sys.modules.pop(name) for name in names if name in sys.modules}
    try:
        song = track_signals.c2_song(SONG_SECONDS, seed=SONG_SEED)
        src = tmp_path / "song.wav"
        _write_wav(src, song)
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "plain"))
        plain = api.last_result()
        assert not [name for name in names if name in sys.modules]
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "wav"), runtime_overrides={"output.format": "wav"})
        named = api.last_result()
        assert not [name for name in names if name in sys.modules]
    finally:
        sys.modules.update(held)
    assert "export_format" not in plain
    rel = [Path(p).relative_to(tmp_path / "plain") for p in plain["saved_files"]]
    assert rel == [Path(p).relative_to(tmp_path / "wav") for p in named["saved_files"]] and all(p.suffix == ".wav" for p in rel)
    for p in rel:
        assert (tmp_path / "plain" / p).read_bytes() == (tmp_path / "wav" / p).read_bytes(), p
    words = np.clip(np.rint(song * 32767.0), -32768, 32767).astype(np.int64)
    pieces = [_wav_words(p)[0][:, 0] for p in plain["mix_segment_files"]]
    assert (np.concatenate(pieces) == words << 8).all()
