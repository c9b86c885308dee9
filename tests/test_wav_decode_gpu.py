"""ac_decode_pcm (include/audiocut_hip_load.h) against `wav_reader.decode_host`, its non-finite count, and `separate_and_segment`
through the device loader.  Every comparison is `np.array_equal` on float32: the arithmetic is exact, there is no tolerance."""
import struct
from pathlib import Path

import numpy as np
import pytest

from audio_cut_amd.utils import wav_reader as WR

pytestmark = pytest.mark.gpu

SR = 44100
KS_TAIL = bytes.fromhex("000000001000800000AA00389B71")
CANARY = np.float32(-777.25)
FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
FRAMES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)       # below a quad, the first pass boundary of a workgroup, more than one workgroup


def _info(fmt, channels, n, rate=SR):
    w = WR.SAMPLE_FORMATS[fmt][1]
    return WR.WavInfo(sample_rate=rate, channels=channels, sample_format=fmt, container_bytes=w, bits_per_sample=8 * w, n_frames=n,
                      data_offset=44, data_bytes=n * channels * w)


def _random_bytes(rng, fmt, count):
    """`count` samples as file bytes: every bit pattern for the integer formats, finite values of many magnitudes for the float ones
    (float64 values that are no float32, so the conversion rounds)."""
    if fmt == "f32":
        return (rng.standard_normal(count) * np.exp(rng.uniform(-20, 4, count))).astype("<f4").view(np.uint8)
    if fmt == "f64":
        return (rng.standard_normal(count) * np.exp(rng.uniform(-20, 4, count))).astype("<f8").view(np.uint8)
    return rng.integers(0, 256, size=count * WR.SAMPLE_FORMATS[fmt][1], dtype=np.uint8)


def _upload(hip, raw, shift):
    """The bytes on the device at a 4-byte aligned address that is `shift` bytes off an allocation's start."""
    import torch
    buf = torch.zeros(shift + raw.size, dtype=torch.uint8, device=hip.device)
    buf[shift:] = hip.to_device(raw)
    return buf[shift:]


@pytest.mark.parametrize("layout", [WR.LAYOUT_MONO, WR.LAYOUT_PLANAR], ids=["mono", "planar"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_matches_decode_host(hip_ctx, fmt, layout):
    import torch
    rng = np.random.default_rng(100 + FORMATS.index(fmt))
    for channels in (1, 2, 3, 6):
        for k, n in enumerate(FRAMES):
            raw = _random_bytes(rng, fmt, n * channels)
            info = _info(fmt, channels, n)
            want = WR.decode_host(raw, info, layout)
            raw_dev = _upload(hip_ctx, raw, 4 * (k % 3))
            if layout == WR.LAYOUT_PLANAR:
                stride = n + 5
                flat = torch.full((channels * stride + 7,), float(CANARY), dtype=torch.float32, device=hip_ctx.device)
                _, bad = hip_ctx.decode_pcm(raw_dev, info, layout, out=flat[: channels * stride].view(channels, stride))
                host = flat.cpu().numpy()
                got = host[: channels * stride].reshape(channels, stride)
                assert np.array_equal(got[:, :n].view(np.uint32), want.view(np.uint32)), (fmt, channels, n)
                assert np.all(got[:, n:] == CANARY) and np.all(host[channels * stride:] == CANARY), (fmt, channels, n)
            else:
                flat = torch.full((n + 7,), float(CANARY), dtype=torch.float32, device=hip_ctx.device)
                _, bad = hip_ctx.decode_pcm(raw_dev, info, layout, out=flat[:n])
                host = flat.cpu().numpy()
                assert np.array_equal(host[:n].view(np.uint32), want.view(np.uint32)), (fmt, channels, n)
                assert np.all(host[n:] == CANARY), (fmt, channels, n)
            assert bad == 0, (fmt, channels, n)
    # without `out`: a fresh tensor of the result's own shape
    info = _info(fmt, 2, 777)
    raw = _random_bytes(rng, fmt, 2 * 777)
    got, bad = hip_ctx.decode_pcm(hip_ctx.to_device(raw), info, layout)
    assert bad == 0 and np.array_equal(got.cpu().numpy(), WR.decode_host(raw, info, layout))


def test_eight_channels_and_the_widest_frame(hip_ctx):
    """8 x float64 = 64 bytes per frame: the 256-frame passes; the mean in channel order is the definition at 8 channels."""
    rng = np.random.default_rng(8)
    for fmt in ("s24", "f64"):
        info = _info(fmt, 8, 1300)
        raw = _random_bytes(rng, fmt, 8 * 1300)
        for layout in (WR.LAYOUT_MONO, WR.LAYOUT_PLANAR):
            got, bad = hip_ctx.decode_pcm(hip_ctx.to_device(raw), info, layout)
            assert bad == 0 and np.array_equal(got.cpu().numpy(), WR.decode_host(raw, info, layout)), (fmt, layout)


def _wav(fmt_tag, channels, rate, width, payload, extensible=False, extra=b""):
    ba = channels * width
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else fmt_tag, channels, rate, rate * ba, ba, 8 * width)
    if extensible:
        body += struct.pack("<HHI", 22, 8 * width, 0) + struct.pack("<H", fmt_tag) + KS_TAIL
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + extra + b"data" + struct.pack("<I", len(payload)) + payload
    chunks += b"\0" * (len(payload) & 1)
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_nonfinite_count_is_exact_and_repeatable(hip_ctx, tmp_path, fmt):
    from audio_cut_amd import api
    n, channels = 1027, 3                                                  # 1027 % 4 == 3: frames 1024..1026 are the last, partial quad
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((n, channels)) * 0.3).astype(np.float64 if fmt == "f64" else np.float32)
    x[0, 0], x[2, 1], x[3, 2] = np.nan, np.inf, -np.inf                    # the first quad, a channel each
    x[1024, 2], x[1025, 0], x[1026, 1] = -np.inf, np.nan, np.inf           # the last three frames
    x[500, 1] = np.nan
    expected = 7
    if fmt == "f64":
        x[1, 1], x[1026, 2], x[700, 0] = 1e39, -1e300, 3.4028235e38        # beyond float32 twice; its largest finite value does not count
        expected = 9
    raw = x.reshape(-1).view(np.uint8)
    info = _info(fmt, channels, n)
    assert WR.count_nonfinite(raw, info) == expected
    raw_dev = hip_ctx.to_device(raw)
    for layout in (WR.LAYOUT_MONO, WR.LAYOUT_PLANAR):
        got, bad = hip_ctx.decode_pcm(raw_dev, info, layout)
        got2, bad2 = hip_ctx.decode_pcm(raw_dev, info, layout)
        assert bad == bad2 == expected, (layout, bad, bad2)
        with np.errstate(invalid="ignore", over="ignore"):
            want = WR.decode_host(raw, info, layout)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)) and np.array_equal(got.cpu().numpy()[fin], want[fin])
        assert np.array_equal(got.cpu().numpy()[~np.isnan(want)], want[~np.isnan(want)])
    p = tmp_path / f"bad_{fmt}.wav"
    p.write_bytes(_wav(3, channels, SR, info.container_bytes, raw.tobytes()))
    with pytest.raises(ValueError, match=f"{expected} samples are NaN or infinite"):
        api.load_audio_device(str(p), hip_ctx, 1)
    # the integer formats cannot hold one: the count stays 0 whatever the bytes
    _, bad = hip_ctx.decode_pcm(raw_dev, _info("s32", channels, n), WR.LAYOUT_MONO)
    assert bad == 0


def test_load_audio_device_is_the_host_loaders_on_the_device(hip_ctx, tmp_path):
    from audio_cut_amd import api
    rng = np.random.default_rng(21)
    list_chunk = b"LIST" + struct.pack("<I", 7) + b"INFOabc" + b"\0"
    files = {
        "s24x_stereo": _wav(1, 2, 48000, 3, rng.integers(0, 256, 6 * 4099, dtype=np.uint8).tobytes(), extensible=True, extra=list_chunk),
        "s16_mono": _wav(1, 1, SR, 2, rng.integers(0, 256, 2 * 1025, dtype=np.uint8).tobytes()),
        "f32_six": _wav(3, 6, SR, 4, rng.standard_normal(6 * 333).astype("<f4").tobytes(), extensible=True),
        "u8_stereo_odd": _wav(1, 2, 8000, 1, rng.integers(0, 256, 2 * 1001 + 1, dtype=np.uint8).tobytes()),    # a trailing half frame
    }
    for name, blob in files.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(blob)
        want, sr = api.load_audio_mono(str(p))
        got, sr_dev = api.load_audio_device(str(p), hip_ctx, 1)
        assert sr_dev == sr and np.array_equal(got.cpu().numpy(), want), name
        if name == "f32_six":
            with pytest.raises(ValueError, match="6 channels; audio.channels: 2 takes mono or stereo input"):
                api.load_audio_device(str(p), hip_ctx, 2)
            continue
        want2, _ = api.load_audio_stereo(str(p))
        got2, _ = api.load_audio_device(str(p), hip_ctx, 2)
        assert got2.is_contiguous() and np.array_equal(got2.cpu().numpy(), want2), name


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def song_files(tmp_path_factory):
    """One 14 s stereo track quantised to 16 bits, as a plain PCM_16 WAV, as an extensible one with a LIST chunk in front of the data,
    and as a float32 WAV holding exactly pcm / 32768."""
    from audio_cut_amd.testing import signals
    st = signals.c2_song(14.0, seed=9, stereo=True)
    pcm = np.clip(np.rint(st.T * 32767.0), -32768, 32767).astype("<i2")
    root = tmp_path_factory.mktemp("wav_decode_e2e")
    list_chunk = b"LIST" + struct.pack("<I", 17) + b"INFOISFT" + struct.pack("<I", 5) + b"abcd\0" + b"\0"
    blobs = {"plain": _wav(1, 2, SR, 2, pcm.tobytes()),
             "ext": _wav(1, 2, SR, 2, pcm.tobytes(), extensible=True, extra=list_chunk),
             "float": _wav(3, 2, SR, 4, (pcm.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes())}
    paths = {}
    for name, blob in blobs.items():
        paths[name] = root / f"song_{name}.wav"
        paths[name].write_bytes(blob)
    return root, paths


_RUNS: dict = {}


def _run(song_files, hip_ctx, name, channels, gpu_decode=True):
    """(cut samples, the bytes of every exported mix segment); each combination runs once per session."""
    key = (name, channels, gpu_decode)
    if key not in _RUNS:
        from audio_cut_amd import api
        root, paths = song_files
        out = root / f"out_{name}_{channels}_{int(gpu_decode)}"
        overrides = {"audio.channels": channels}
        if not gpu_decode:
            overrides["audio.gpu_decode"] = False
        man = api.separate_and_segment(input_uri=str(paths[name]), export_dir=str(out), export_types=["mix_segments"],
                                       runtime_overrides=overrides)
        files = api.last_result()["mix_segment_files"]
        assert man["success"] and len(files) == man["stats"]["num_segments"] >= 1 and man["audio"]["channels"] == channels
        assert man["audio"]["duration"] == man["cuts"]["samples"][-1] / SR
        _RUNS[key] = (list(man["cuts"]["samples"]), [Path(f).name for f in files], [Path(f).read_bytes() for f in files])
    return _RUNS[key]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name,gpu_decode", [("plain", False), ("ext", True), ("float", True)], ids=["host_decode", "extensible", "float32"])
def test_end_to_end_same_cuts_and_bytes_as_the_plain_file_on_the_device(hip_ctx, song_files, name, gpu_decode, channels):
    """The plain PCM_16 file through the device loader is the reference of its channel count (run once and shared).  The same file
    with `audio.gpu_decode` off - the old path against the new -, the extensible copy and the float32 copy give the same cut samples
    and the same bytes in every exported mix segment."""
    ref = _run(song_files, hip_ctx, "plain", channels)
    assert ref[0][0] == 0 and len(ref[0]) >= 2 and len(ref[2]) >= 1
    got = _run(song_files, hip_ctx, name, channels, gpu_decode=gpu_decode)
    assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2]
