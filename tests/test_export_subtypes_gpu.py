"""The export subtypes on the GPU: `ac_pack_pcm` and `ac_mdx_assemble_pcm` (include/audiocut_hip_pack.h) bit for bit against the host
conversion and against the 24-bit entry points they generalise, and `output.wav.subtype` end to end.

`ac_pack_pcm`: every subtype, mono and stereo, at frame counts that give every length of the last (partial) group, an odd stereo
track, one workgroup and more than one (1023 and 1025 frames are 256 and 257 groups of a mono track), a stereo track in rows wider
than the track (even stride: the 8-byte loads; odd stride: row 1 is not 8-byte aligned, the sample-by-sample loads) and a mono
track that is not 16-byte aligned.  The inputs hold the known answers of tests/test_export_subtypes_host.py at all four positions
of a group.  Sixteen sentinel bytes behind the output must keep their value.

`ac_mdx_assemble_pcm`: a hand-made plan of two chunks whose effective regions overlap and leave the tail of the track uncovered, on
a track of 2311 frames (n % 4 == 3, an odd stereo track, three workgroups of a mono track), against `pack_pcm(mdx_assemble_ola(..))`.

End to end the float files of a FLOAT run, decoded and converted on the host, must be the files of the default and of the PCM_16
run: the pipeline gives the same stems in every run, only the last conversion differs."""
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import mdx_refs as R
from audio_cut_amd.testing import signals
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import wav_reader as WR

pytestmark = pytest.mark.gpu

SR = 44100
ITEM = R.ITEM
SUBTYPES = ("PCM_U8", "PCM_16", "PCM_24", "PCM_32", "FLOAT", "DOUBLE")
WIDTH = {"PCM_U8": 1, "PCM_16": 2, "PCM_24": 3, "PCM_32": 4, "FLOAT": 4, "DOUBLE": 8}
FRAMES = (1, 2, 3, 4, 5, 7, 1023, 1025)
# the known answers of the host test, then a denormal, -0.0 and the infinities (FLOAT keeps them, the integer subtypes clip them)
KNOWN_X = np.array([0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, np.nan, 0.9 * 2.0 ** -7, -0.1 * 2.0 ** -7, 1e-45, -0.0, np.inf, -np.inf],
                   dtype=np.float32)
SENTINEL = 0xA5


def _input(n: int, channels: int, rotation: int) -> np.ndarray:
    """Planar [channels, n] noise of scale 0.6 clipped to +-1.3 with KNOWN_X at the interleaved words rotation, rotation + 1, ..."""
    rng = np.random.default_rng(1000 * n + 10 * channels + rotation)
    words = np.clip(0.6 * rng.standard_normal(n * channels), -1.3, 1.3).astype(np.float32)      # frame-interleaved
    k = max(0, min(KNOWN_X.size, words.size - rotation))
    words[rotation: rotation + k] = KNOWN_X[:k]
    return np.ascontiguousarray(words.reshape(n, channels).T)


def _bits(a: np.ndarray) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def _pack_checked(hip, xd: torch.Tensor, subtype: str) -> np.ndarray:
    """pack_pcm_device into a buffer with 16 sentinel bytes behind the sample bytes, which must survive."""
    n_bytes = int(xd.shape[-1]) * xd.dim() * WIDTH[subtype]
    out = torch.full((n_bytes + 16,), SENTINEL, dtype=torch.uint8, device=hip.device)
    got = hip.pack_pcm_device(xd, subtype, out=out)
    assert got.numel() == n_bytes and got.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    assert (host[n_bytes:] == SENTINEL).all(), f"{subtype}: bytes behind the output were written"
    return host[:n_bytes]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("subtype", SUBTYPES)
def test_pack_pcm_against_the_host_conversion(hip_ctx, subtype, channels):
    for n in FRAMES:
        for rotation in range(4):
            x = _input(n, channels, rotation)                       # [channels, n]
            want, width = AE.pcm_bytes_host(x.T, subtype)
            assert width == WIDTH[subtype]
            xd = hip_ctx.to_device(x if channels == 2 else x[0])
            got = _pack_checked(hip_ctx, xd, subtype)
            assert got.tobytes() == want.tobytes(), (subtype, channels, n, rotation)
            if rotation == 0:
                assert hip_ctx.pack_pcm(xd, subtype).tobytes() == want.tobytes()
            if subtype == "PCM_24":                                 # the new entry point writes what the old one writes
                old = hip_ctx.pack_pcm24(xd.t().contiguous().reshape(-1) if channels == 2 else xd)
                assert got.tobytes() == old.tobytes(), (channels, n, rotation)


@pytest.mark.parametrize("subtype", SUBTYPES)
def test_pack_pcm_rows_and_alignment(hip_ctx, subtype):
    """A stereo track whose rows stand in wider rows (nothing is copied): an even stride keeps the 8-byte loads, an odd one puts row
    1 off 8-byte alignment and takes the sample-by-sample loads, as does a track that starts at an odd sample; a mono track that
    starts one sample into its buffer is not 16-byte aligned.  All are converted, none refused, and the gap between the rows is
    not read as samples."""
    for n, stride, offset in ((1025, 1032, 0), (1025, 1031, 0), (7, 9, 0), (1025, 1032, 1), (5, 6, 0)):
        x = _input(n, 2, n % 4)
        base = torch.full((2, stride + offset), 7.0, dtype=torch.float32, device=hip_ctx.device)
        base[:, offset: offset + n] = hip_ctx.to_device(x)
        xd = base[:, offset: offset + n]
        assert xd.stride(0) == stride + offset and not xd.is_contiguous()
        want, _ = AE.pcm_bytes_host(x.T, subtype)
        assert _pack_checked(hip_ctx, xd, subtype).tobytes() == want.tobytes(), (subtype, n, stride, offset)
    for n, offset in ((1025, 1), (1023, 3), (6, 2)):
        x = _input(n, 1, 1)[0]
        base = torch.zeros(n + offset, dtype=torch.float32, device=hip_ctx.device)
        base[offset:] = hip_ctx.to_device(x)
        want, _ = AE.pcm_bytes_host(x, subtype)
        assert _pack_checked(hip_ctx, base[offset:], subtype).tobytes() == want.tobytes(), (subtype, n, offset)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("subtype", ["PCM_24", "PCM_16"])
def test_packed_track_on_a_device_track(hip_ctx, subtype, channels):
    """`PackedTrack` with a context and a device track (one `ac_pack_pcm` launch on the planar track as it is, for every subtype)
    holds the bytes of `PackedTrack` without a context (the host conversion).  A stereo track once contiguous and once as rows
    that are views into wider rows, at an even stride (the 8-byte loads) and an odd one (sample by sample); the frame counts give
    a lone partial group, full groups, and a partial last group in a workgroup of its own (1025 frames).  Stereo PCM_24 used to be
    transposed on the device and packed as 2N mono samples: that route, rebuilt here, gives the same bytes."""
    for n in (1, 2, 3, 4, 5, 1025):
        x = _input(n, channels, n % 4)                              # [channels, n]
        x_host = x if channels == 2 else x[0]
        want = AE.PackedTrack(x_host, SR, subtype)
        tracks = [hip_ctx.to_device(x_host)]
        if channels == 2:
            for stride in (n + n % 2 + 2, n + n % 2 + 3):
                base = torch.full((2, stride), 7.0, dtype=torch.float32, device=hip_ctx.device)
                base[:, :n] = tracks[0]
                tracks.append(base[:, :n])
                assert tracks[-1].stride(0) == stride and not tracks[-1].is_contiguous()
        for xd in tracks:
            got = AE.PackedTrack(x_host, SR, subtype, hip=hip_ctx, dev=xd)
            assert (got.n, got.channels, got.width, got.subtype) == (want.n, want.channels, want.width, want.subtype) == \
                (n, channels, WIDTH[subtype], subtype)
            assert np.asarray(got.bytes).tobytes() == np.asarray(want.bytes).tobytes(), (subtype, channels, n, xd.stride(0))
            if channels == 2 and subtype == "PCM_24":
                old = hip_ctx.pack_pcm24(xd.t().contiguous().reshape(-1))
                assert np.asarray(got.bytes).tobytes() == old.tobytes(), (n, xd.stride(0))


def test_pack_pcm_wrapper_refusals(hip_ctx):
    from audio_cut_amd import _native
    dev = hip_ctx.device
    x = torch.zeros(8, device=dev)
    with pytest.raises(ValueError, match="ULAW"):
        hip_ctx.pack_pcm(x, "ULAW")
    for bad in (torch.zeros((3, 8), device=dev), torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(0, device=dev),
                torch.zeros(16, device=dev)[::2], torch.zeros((2, 2, 2), device=dev)):
        with pytest.raises(_native.NativeError):
            hip_ctx.pack_pcm(bad, "PCM_16")
    with pytest.raises(_native.NativeError):
        hip_ctx.pack_pcm_device(x, "PCM_32", out=torch.zeros(31, dtype=torch.uint8, device=dev))
    with pytest.raises(_native.NativeError, match="aligned"):        # the library's own check: a PCM_32 stream needs 16 bytes
        hip_ctx.pack_pcm_device(x, "PCM_32", out=torch.zeros(64, dtype=torch.uint8, device=dev)[4:])


# ---- ac_mdx_assemble_pcm ------------------------------------------------------------------------------------------------------
# (chunk_start, chunk_end, eff_start, eff_end): the effective regions overlap in [800, 1000) and nothing covers [2100, 2311)
ASSEMBLE_N = 2311
ASSEMBLE_RANGES = [(0, 1500, 0, 1000), (800, 2300, 800, 2100)]


@pytest.fixture(scope="module")
def assemble_case(hip_ctx):
    """Per channel count: the device track, waves and tables, the float stems of mdx_assemble_ola and the 24-bit results."""
    cases = {}
    cnt = R.coverage(ASSEMBLE_N, ASSEMBLE_RANGES)
    assert (int(cnt.max()), int(cnt[2100:].max()), int(cnt[:2100].min())) == (2, 0, 1)
    c_start, c_len, c_es, c_ee, c_base = R.chunk_tables(ASSEMBLE_RANGES)
    n_items = len(R.item_tables(ASSEMBLE_RANGES)[0])
    assert n_items == 2 and c_base.tolist() == [0, 1]
    for stereo in (False, True):
        rng = np.random.default_rng(ASSEMBLE_N + stereo)
        x = 0.3 * rng.standard_normal((2, ASSEMBLE_N) if stereo else ASSEMBLE_N, dtype=np.float32)
        wave_h = rng.standard_normal((n_items, 2, ITEM), dtype=np.float32) * np.float32(0.6)    # one sample in ten clips
        xd, wd = hip_ctx.to_device(x), hip_ctx.to_device(wave_h)
        tables = [hip_ctx.to_device(a) for a in (c_start, c_len, c_es, c_ee, c_base)]
        v, i, vs, is_ = hip_ctx.mdx_assemble_ola(xd, wd, *tables)
        stem24, rest24, parts24 = hip_ctx.mdx_assemble_pcm24(xd, wd, *tables)
        cases[stereo] = dict(xd=xd, wd=wd, tables=tables, stem=vs if stereo else v, rest=is_ if stereo else i,
                             stem24=stem24.cpu().numpy(), rest24=rest24.cpu().numpy(), parts24=parts24.cpu().numpy())
    return cases


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("subtype", SUBTYPES)
def test_assemble_pcm_against_assemble_then_pack(hip_ctx, assemble_case, subtype, stereo):
    c = assemble_case[stereo]
    ch = 2 if stereo else 1
    stem_d, rest_d, parts_d = hip_ctx.mdx_assemble_pcm(c["xd"], c["wd"], *c["tables"], subtype)
    assert stem_d.dtype == rest_d.dtype == torch.uint8 and stem_d.numel() == rest_d.numel() == WIDTH[subtype] * ch * ASSEMBLE_N
    stem, rest, parts = stem_d.cpu().numpy(), rest_d.cpu().numpy(), parts_d.cpu().numpy()
    assert stem.tobytes() == hip_ctx.pack_pcm(c["stem"], subtype).tobytes(), "stem bytes differ from pack_pcm(mdx_assemble_ola)"
    assert rest.tobytes() == hip_ctx.pack_pcm(c["rest"], subtype).tobytes(), "rest bytes differ from pack_pcm(mdx_assemble_ola)"
    # and the float stems through the host conversion
    for got, stem_f in ((stem, c["stem"]), (rest, c["rest"])):
        host = stem_f.cpu().numpy()
        assert got.tobytes() == AE.pcm_bytes_host(host.T if stereo else host, subtype)[0].tobytes()
    # the partial sums do not depend on the subtype: those of the 24-bit entry point, bit for bit
    assert parts.shape == c["parts24"].shape and _bits(parts) == _bits(c["parts24"])
    if subtype == "PCM_24":
        assert stem.tobytes() == c["stem24"].tobytes() and rest.tobytes() == c["rest24"].tobytes()
    if subtype in ("PCM_U8", "PCM_16", "PCM_32"):                    # both clip limits are reached
        w = stem.view({"PCM_U8": np.uint8, "PCM_16": "<i2", "PCM_32": "<i4"}[subtype])
        assert w.min() == np.iinfo(w.dtype).min and w.max() == np.iinfo(w.dtype).max
    # the uncovered tail is silence in every subtype's own spelling
    frame = WIDTH[subtype] * ch
    tail = stem.reshape(ASSEMBLE_N, frame)[2100:]
    assert (tail == (128 if subtype == "PCM_U8" else 0)).all()


def test_assemble_pcm_wrapper_refusals(hip_ctx):
    from audio_cut_amd import _native
    dev = hip_ctx.device
    t = [torch.zeros(1, dtype=torch.int64, device=dev)] * 4 + [torch.zeros(1, dtype=torch.int32, device=dev)]
    w = torch.zeros((1, 2, ITEM), device=dev)
    with pytest.raises(ValueError, match="ALAW"):
        hip_ctx.mdx_assemble_pcm(torch.zeros(8, device=dev), w, *t, "ALAW")
    for bad in (torch.zeros((3, 8), device=dev), torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(0, device=dev)):
        with pytest.raises(_native.NativeError):
            hip_ctx.mdx_assemble_pcm(bad, w, *t, "FLOAT")


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _write_wav(path, x):
    pcm = np.clip(np.rint(x * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())


def _files(root: Path):
    """{relative name: (WavInfo, sample bytes)} of every file under `root`."""
    out = {}
    for p in sorted(root.rglob("*")):
        if p.is_file():
            assert p.suffix == ".wav", p
            info = WR.read_wav_info(p)
            out[p.relative_to(root).as_posix()] = (info, WR.read_wav_bytes(p, info))
    return out


def _assert_same_audio(float_files, other_files, subtype):
    """Every FLOAT file, decoded and converted on the host, is the other run's file of the same name."""
    fmt = {"PCM_24": "s24", "PCM_16": "s16"}[subtype]
    assert list(float_files) == list(other_files) and float_files
    for name, (info, raw) in float_files.items():
        o_info, o_raw = other_files[name]
        assert info.sample_format == "f32" and info.data_offset == 56 and o_info.sample_format == fmt and o_info.data_offset == 44, name
        assert (info.n_frames, info.channels, info.sample_rate) == (o_info.n_frames, o_info.channels, o_info.sample_rate), name
        want, _ = AE.pcm_bytes_host(WR.decode_samples(raw, info), subtype)
        assert want.tobytes() == o_raw.tobytes(), f"{name}: the {subtype} file is not the conversion of the FLOAT file"


@pytest.fixture(scope="module")
def song_path(tmp_path_factory):
    src = tmp_path_factory.mktemp("subtype_song") / "song.wav"
    _write_wav(src, signals.c2_song(14.0, seed=9))
    return src


def test_subtype_end_to_end(hip_ctx, tmp_path, song_path):
    """Three runs of the default mode: nothing set, FLOAT, PCM_16.  The same names, cuts and frame counts; every FLOAT file is,
    converted on the host, the default run's PCM_24 file and the PCM_16 run's file."""
    from audio_cut_amd import api, config
    runs = {}
    for key, over in (("default", None), ("FLOAT", {"output.wav.subtype": "FLOAT"}), ("PCM_16", {"output.wav.subtype": "PCM_16"})):
        man = api.separate_and_segment(input_uri=str(song_path), export_dir=str(tmp_path / key), runtime_overrides=over)
        res = api.last_result()
        assert res["success"] is True
        runs[key] = (_files(tmp_path / key), res, man)
        assert config.get_config("output.wav.subtype") == "PCM_24"           # the override does not outlive the call
    files = {k: v[0] for k, v in runs.items()}
    res = runs["default"][1]
    assert res["mix_segment_files"] and res["full_vocal_file"] and res["full_instrumental_file"]
    assert len(files["default"]) == len(res["saved_files"])
    for key in ("FLOAT", "PCM_16"):                                             # no new keys, the same names, cuts and counts
        assert set(runs[key][1]) == set(res) and set(runs[key][2]) == set(runs["default"][2])
        assert runs[key][1]["cut_points_samples"] == res["cut_points_samples"]
        assert [Path(p).relative_to(tmp_path / key) for p in runs[key][1]["saved_files"]] == \
            [Path(p).relative_to(tmp_path / "default") for p in res["saved_files"]]
    _assert_same_audio(files["FLOAT"], files["default"], "PCM_24")
    _assert_same_audio(files["FLOAT"], files["PCM_16"], "PCM_16")
    with pytest.raises(ValueError, match="mp3"):
        api.separate_and_segment(input_uri=str(song_path), export_dir=str(tmp_path / "mp3"), runtime_overrides={"output.format": "mp3"})


def test_subtype_end_to_end_vocal_separation(hip_ctx, tmp_path, song_path):
    """Mode `vocal_separation` (the fused writer): the PCM_16 run's stems are the host conversion of the FLOAT run's."""
    from audio_cut_amd import api
    sep = {}
    for key in ("FLOAT", "PCM_16"):
        api.separate_and_segment(input_uri=str(song_path), export_dir=str(tmp_path / key), mode="vocal_separation",
                                 runtime_overrides={"output.wav.subtype": key})
        sep[key] = _files(tmp_path / key)
        res = api.last_result()
        assert res["method"] == "vocal_separation_only" and "subtype" not in res and len(res["saved_files"]) == 2
    assert len(sep["FLOAT"]) == 2
    _assert_same_audio(sep["FLOAT"], sep["PCM_16"], "PCM_16")
