"""`output.sample_rate` on the host (audio_cut_amd/utils/rate_export.py): how the setting resolves and what it refuses, the cut
mapping, the host statement of the resampled bytes against scipy.signal.resample_poly with the same taps, the lossless round trip
of a file's own data chunk, and the bad arguments the entry point of include/audiocut_hip_rate.h refuses.  CPU only."""
import ctypes as C
import struct
import wave

import numpy as np
import pytest

import resample_refs as R
from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd import _native, api, config
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import rate_export as RE
from audio_cut_amd.utils import wav_reader as WR

SR = 44100


# ---- the setting ---------------------------------------------------------------------------------------------------------------------
def test_resolve_output_rate():
    saved = config.snapshot()
    try:
        assert config.get_config("output.sample_rate", None) is None
        assert RE.resolve_output_rate(48000, SR) == SR and RE.resolve_output_rate(None, SR) == SR        # absent: the pipeline rate
        config.set_runtime_config({"output.sample_rate": "source"})
        assert RE.resolve_output_rate(48000, SR) == 48000 and RE.resolve_output_rate(96000, SR) == 96000
        assert RE.resolve_output_rate(SR, SR) == SR
        assert RE.resolve_output_rate(None, SR) == SR                                                    # a .npy input has no rate
        with pytest.raises(ValueError, match="'source'.*44101"):
            RE.resolve_output_rate(44101, SR)
        config.set_runtime_config({"output.sample_rate": 96000})
        assert RE.resolve_output_rate(48000, SR) == 96000 and RE.resolve_output_rate(None, SR) == 96000
        config.set_runtime_config({"output.sample_rate": None})
        assert RE.resolve_output_rate(48000, SR) == SR
    finally:
        config.restore(saved)
    assert config.get_config("output.sample_rate", None) is None


def test_the_bound_admits_the_usual_rates_and_keeps_the_filter_small():
    for rate in (8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000, 176400, 192000, 384000):
        assert RE.check_output_rate(rate, SR) == rate and max(RE.rate_ratio(rate, SR)) <= RE.MAX_RATIO_TERM == 1280
    assert RE.rate_ratio(384000, SR) == (1280, 147) and RE.rate_ratio(48000, SR) == (160, 147) and RE.rate_ratio(SR, 48000) == (147, 160)
    assert _native.Context._resample_filter(1280, 147)[0].size <= 245_000


REFUSED = [44100.0, 48000.5, "48k", "Source", "", True, False, 0, -48000, 44101, 7, 768000, [48000], {"hz": 48000}]


def _tiny_wav(path, rate=SR):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate); w.writeframes(np.zeros(64, "<i2").tobytes())
    return path


@pytest.mark.parametrize("value", REFUSED, ids=[repr(v) for v in REFUSED])
def test_api_refuses_the_rate_before_any_work(tmp_path, value):
    """A refused value raises ValueError naming it before the track is loaded or a device is touched (there is none on this
    machine: getting any further would fail differently), nothing is written and the configuration is put back."""
    src = _tiny_wav(tmp_path / "in.wav")
    with pytest.raises(ValueError) as err:
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), runtime_overrides={"output.sample_rate": value})
    assert "output.sample_rate" in str(err.value) and repr(value) in str(err.value)
    assert config.get_config("output.sample_rate", None) is None
    assert not list((tmp_path / "out").iterdir())


def test_api_refuses_a_source_rate_it_cannot_resample_to_and_vocal_separation(tmp_path):
    src = _tiny_wav(tmp_path / "odd.wav", rate=44101)
    with pytest.raises(ValueError, match="'source'") as err:
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), runtime_overrides={"output.sample_rate": "source"})
    assert "44101" in str(err.value)
    src48 = _tiny_wav(tmp_path / "in48.wav", rate=48000)
    for value in ("source", 96000):
        with pytest.raises(ValueError, match="vocal_separation") as err:
            api.separate_and_segment(input_uri=str(src48), export_dir=str(tmp_path / "out"), mode="vocal_separation",
                                     runtime_overrides={"output.sample_rate": value})
        assert "v2.2_mdd" in str(err.value) and "full_vocal" in str(err.value) and "full_instrumental" in str(err.value)
    assert config.get_config("output.sample_rate", None) is None
    assert not list((tmp_path / "out").iterdir())


def test_the_key_has_no_default():
    assert config.DEFAULTS["output"] == {"format": "wav", "wav": {"subtype": "PCM_24"}}
    assert config.get_config("output.sample_rate", None) is None and config.get_config("output.sample_rate", "x") == "x"


# ---- the cut mapping -----------------------------------------------------------------------------------------------------------------
def test_map_cut_endpoints_and_the_known_pair():
    n = 617400                                                       # 14 s at 44.1 kHz
    n_out = RE.resampled_len(n, 160, 147)
    assert n_out == 672000
    assert RE.map_cut(0, SR, 48000, n_out) == 0 and RE.map_cut(n, SR, 48000, n_out) == n_out
    assert RE.map_cut(SR, SR, 48000, n_out) == 48000 and RE.map_cut(147, SR, 48000, n_out) == 160
    assert RE.map_cut(1, SR, 48000, n_out) == 1 and RE.map_cut(2, SR, 48000, n_out) == 2 and RE.map_cut(6, SR, 48000, n_out) == 7
    assert RE.map_cut(10 ** 9, SR, 48000, n_out) == n_out           # never past the converted track
    # the end of the track is the end of the converted track, also where the rounded value lies below ceil(n up / down)
    n = 1000
    n_out = RE.resampled_len(n, 320, 147)
    assert n_out == 2177 and (n * 96000 + SR // 2) // SR == 2177
    n = 1001
    n_out = RE.resampled_len(n, 320, 147)
    assert n_out == 2180 and RE.map_cut(n, SR, 96000, n_out) == 2179 and RE.map_cut(n, SR, 96000, n_out, n) == n_out
    assert RE.map_cut(n - 1, SR, 96000, n_out, n) == RE.map_cut(n - 1, SR, 96000, n_out)


@pytest.mark.parametrize("rate", [16000, 22050, 32000, 48000, 96000])
def test_map_cut_is_monotone_and_within_half_a_sample(rate):
    n = 3 * SR + 17
    n_out = RE.resampled_len(n, *RE.rate_ratio(rate, SR))
    c = np.arange(n + 1)
    got = np.array([RE.map_cut(int(v), SR, rate, n_out, n) for v in c])
    assert got[0] == 0 and got[-1] == n_out and np.all(np.diff(got) >= 0)
    exact = c[:-1].astype(np.float64) * rate / SR                     # the end of the track goes to n_out by rule
    assert np.all(np.abs(got[:-1] - exact) <= 0.5) and np.all(got <= n_out)


def test_the_source_round_trip_never_pads():
    """48 kHz -> 44.1 kHz -> 48 kHz: the stems at the file's rate have at least the file's frames, at most two more."""
    n_src = np.arange(1, 200001, dtype=np.int64)
    n = -(-n_src * 147 // 160)
    back = -(-n * 160 // 147)
    assert np.all(back >= n_src) and np.all(back - n_src <= 2)


# ---- the host statement of the bytes -------------------------------------------------------------------------------------------------
def _scipy_window(hfull, up, down, n_pre_remove):
    """`Context._resample_filter` returns scipy's framing (front-padded, scaled by up); scipy wants the bare odd filter at unit
    gain and applies that framing itself."""
    for n_pre_pad in range(1, down + 1):
        h = hfull[n_pre_pad:]
        half_len = (h.size - 1) // 2
        if h.size % 2 == 1 and down - half_len % down == n_pre_pad and (half_len + n_pre_pad) // down == n_pre_remove:
            assert not np.any(hfull[:n_pre_pad])
            return h.astype(np.float64) / up
    raise AssertionError("not scipy.signal.resample_poly's framing")


@pytest.mark.parametrize("up,down", [(160, 147), (147, 160), (320, 147), (2, 1), (1, 2)])
def test_resample_pack_host_is_scipy_resample_poly_with_the_same_taps(up, down):
    import scipy.signal
    hfull, npr = _native.Context._resample_filter(up, down)
    tpp = -(-hfull.size // up)
    window = _scipy_window(hfull, up, down, npr)
    rng = np.random.default_rng(up * 1000 + down)
    for n in (1, 7, tpp - 1, tpp + 1, 2 * tpp + 5):
        x = (rng.standard_normal((2, n)) * 0.3).astype(np.float32)
        n_out = R.n_out_of(n, up, down)
        for crop in (0, 1):
            if n_out - crop < 1:
                continue
            got = np.stack([RE.resample_host(ch, up, down, n_out - crop) for ch in x])
            for c in range(2):
                ref = scipy.signal.resample_poly(x[c].astype(np.float64), up, down, window=window)[: n_out - crop]
                _, mag = R.polyphase_ref64(x[c], up, down, hfull, npr, n_out - crop)
                R.assert_same_taps(got[c], ref, mag, tpp, f"{up}/{down} n {n}", quiet=True)
                # and the correctly rounded reference itself
                y, _ = R.polyphase_ref64(x[c], up, down, hfull, npr, n_out - crop)
                R.assert_same_taps(got[c], y, mag, tpp, f"{up}/{down} n {n} (ref64)", quiet=True)
            # the bytes are pcm_bytes_host of those floats, stereo interleaved, and PCM_16 of scipy's floats is at most 1 LSB away
            for subtype in AE.WAV_SUBTYPES:
                assert np.array_equal(RE.resample_pack_host(x, up, down, subtype, n_out - crop), AE.pcm_bytes_host(got.T, subtype)[0])
                assert np.array_equal(RE.resample_pack_host(x[0], up, down, subtype, n_out - crop), AE.pcm_bytes_host(got[0], subtype)[0])
            ref16 = np.stack([scipy.signal.resample_poly(ch.astype(np.float64), up, down, window=window)[: n_out - crop] for ch in x])
            want = AE.pcm_bytes_host(ref16.astype(np.float32).T, "PCM_16")[0].view("<i2").astype(np.int64)
            have = RE.resample_pack_host(x, up, down, "PCM_16", n_out - crop).view("<i2").astype(np.int64)
            assert np.max(np.abs(have - want)) <= 1


def test_resample_host_edges():
    with pytest.raises(ValueError, match="n_out"):
        RE.resample_host(np.zeros(10, np.float32), 160, 147, 12)          # ceil(10 * 160 / 147) = 11
    with pytest.raises(ValueError, match="n_out"):
        RE.resample_host(np.zeros(10, np.float32), 160, 147, 0)
    with pytest.raises(ValueError, match="ULAW"):
        RE.resample_pack_host(np.zeros(10, np.float32), 160, 147, "ULAW", 11)
    with pytest.raises(ValueError, match="shape"):
        RE.resample_pack_host(np.zeros((3, 10), np.float32), 160, 147, "PCM_16", 11)
    x = np.float32([0.25, -0.5, 1.5, -2.0, 0.0])
    assert np.array_equal(RE.resample_pack_host(x, 3, 3, "PCM_16", 4), AE.pcm_bytes_host(x[:4], "PCM_16")[0])     # equal rates: cropped
    # zeros keep the sign IEEE addition started at -0.0 gives them: a lone -0.0 under a positive tap stays -0.0
    hfull, npr = _native.Context._resample_filter(2, 1)
    y = RE.resample_host(np.float32([-0.0]), 2, 1, 2)
    i0 = npr * 1
    assert hfull[i0] > 0 and np.signbit(y[0]) and y[0] == 0.0
    assert not np.any(np.signbit(RE.resample_host(np.zeros(5, np.float32), 2, 1, 10)[[0, 2, 4, 6, 8]]))  # +0.0 under any tap sum of mixed signs


# ---- lossless: the file's own data chunk -------------------------------------------------------------------------------------------------
def _random_raw(fmt: str, n_frames: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    width = WR.SAMPLE_FORMATS[fmt][1]
    raw = rng.integers(0, 256, size=n_frames * 2 * width, dtype=np.uint8)
    if fmt == "f32":                                                  # finite floats only: the loader refuses a file with NaN or Inf
        bits = raw.view("<u4")
        bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
    return raw


@pytest.mark.parametrize("fmt,subtype", [("u8", "PCM_U8"), ("s16", "PCM_16"), ("s24", "PCM_24"), ("f32", "FLOAT")])
def test_the_data_chunk_comes_back_byte_for_byte(tmp_path, fmt, subtype):
    """A two-channel file decoded as the loader decodes it and packed with the matching subtype is its own data chunk, also in
    pieces: the segments of a track at the file's rate, cut at `map_cut`'s frames, concatenate to it."""
    n_frames, width = 4801, WR.SAMPLE_FORMATS[fmt][1]
    raw = _random_raw(fmt, n_frames, seed=width)
    info = WR.WavInfo(sample_rate=48000, channels=2, sample_format=fmt, container_bytes=width, bits_per_sample=8 * width,
                      n_frames=n_frames, data_offset=44, data_bytes=raw.size)
    planar = WR.decode_host(raw, info, WR.LAYOUT_PLANAR)
    assert np.array_equal(AE.pcm_bytes_host(planar.T, subtype)[0], raw)
    track = AE.PackedTrack(planar, 48000, subtype)
    n = -(-n_frames * 147 // 160)                                     # the pipeline's length of this file
    cuts = [0, 1000, 1001, 2500, n]
    ends = [RE.map_cut(c, SR, 48000, n_frames, n) for c in cuts]
    assert ends[0] == 0 and ends[-1] == n_frames
    pieces = b""
    for i, (lo, hi) in enumerate(zip(ends[:-1], ends[1:])):
        blob = track.write(tmp_path / f"s{i}.wav", lo, hi).read_bytes()
        head = len(AE.wav_header(hi - lo, 48000, 2, width, subtype))
        assert struct.unpack_from("<I", blob, 24)[0] == 48000
        pieces += blob[head: head + (hi - lo) * 2 * width]
    assert pieces == raw.tobytes()


def test_s32_is_the_documented_exception():
    """int32 -> float32 rounds, so a 32-bit PCM file does not come back byte for byte as PCM_32."""
    raw = _random_raw("s32", 4801, seed=32)
    info = WR.WavInfo(sample_rate=48000, channels=2, sample_format="s32", container_bytes=4, bits_per_sample=32, n_frames=4801,
                      data_offset=44, data_bytes=raw.size)
    planar = WR.decode_host(raw, info, WR.LAYOUT_PLANAR)
    assert not np.array_equal(AE.pcm_bytes_host(planar.T, "PCM_32")[0], raw)


def test_packed_track_resampled_on_the_host(tmp_path):
    x = (np.random.default_rng(5).standard_normal((2, 500)) * 0.4).astype(np.float32)
    n_out = RE.resampled_len(500, 160, 147) - 1
    track = AE.PackedTrack.resampled(x, SR, 48000, n_out, "PCM_24")
    assert (track.sample_rate, track.n, track.channels, track.width, track.subtype) == (48000, n_out, 2, 3, "PCM_24")
    assert np.array_equal(track.bytes, RE.resample_pack_host(x, 160, 147, "PCM_24", n_out))
    blob = track.write(tmp_path / "t.wav").read_bytes()
    assert blob == AE.wav_header(n_out, 48000, 2, 3, "PCM_24") + track.bytes.tobytes()
    same = AE.PackedTrack.resampled(x[0], SR, SR, 400, "PCM_16")      # equal rates: the constructor's bytes, cropped
    assert np.array_equal(same.bytes, AE.PackedTrack(x[0][:400], SR, "PCM_16").bytes) and same.n == 400


# ---- the manifest block ----------------------------------------------------------------------------------------------------------------
def test_manifest_export_block_only_with_the_setting(tmp_path):
    src = _tiny_wav(tmp_path / "in.wav")
    base = {"success": True, "cut_points_samples": [0, 64], "cut_points_sec": [0.0, 64 / SR], "num_segments": 1}
    kw = dict(input_path=src, export_dir=tmp_path, mode="v2.2_mdd", sample_rate=SR, channels=1, layout_cfg={})
    assert "export" not in api._build_manifest(result=base, **kw)
    man = api._build_manifest(result={**base, "export_sample_rate": 48000, "source_sample_rate": 48000,
                                      "export_cut_points_samples": [0, 70]}, **kw)
    assert man["export"] == {"sr": 48000, "source_sr": 48000, "cuts_samples": [0, 70]}
    assert man["audio"]["sr"] == SR and man["cuts"]["samples"] == [0, 64]


# ---- include/audiocut_hip_rate.h -------------------------------------------------------------------------------------------------------
def test_rate_entry_point_rejects_bad_arguments(lib):
    """Every refusal comes back as AC_E_INVALID with a message, before anything is launched.  The checks never read the context or
    the buffers, so placeholders stand in for them here (no device on this machine)."""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    raw = C.create_string_buffer(256)
    addr = (C.addressof(raw) + 15) & ~15
    buf, odd, off2, off4, off8 = (C.c_void_p(addr + k) for k in (0, 1, 2, 4, 8))
    call = lib.ac_resample_poly_pack
    # x, n, channels, row_stride, up, down, hp, hlen, n_pre_remove, subtype, out, n_out
    good = [buf, 100, 2, 100, 160, 147, buf, 160 * 10, 5, 4, buf, 109]          # ceil(100 * 160 / 147) = 109

    def changed(*pairs):
        args = list(good)
        for index, value in pairs:
            args[index] = value
        return [ctx] + args

    cases = [([None] + good, "null"), (changed((0, None)), "null"), (changed((6, None)), "null"), (changed((10, None)), "null"),
             (changed((1, 0)), "sizes"), (changed((4, 0)), "sizes"), (changed((5, -1)), "sizes"), (changed((7, 0)), "sizes"),
             (changed((8, -1)), "sizes"), (changed((11, 0)), "sizes"), (changed((11, -3)), "sizes"),
             (changed((7, 160 * 10 + 1)), "polyphase rows"),
             (changed((2, 0)), "channels"), (changed((2, 3)), "channels"), (changed((3, 99)), "row_stride"),
             (changed((1, 1 << 61), (3, 1 << 61)), "too long"), (changed((8, 1 << 61)), "too long"),
             (changed((11, 110)), "n_out"), (changed((11, 1 << 40)), "n_out"),
             (changed((9, 6)), "subtype"), (changed((9, -1)), "subtype"),
             (changed((0, off2)), "4-byte"), (changed((0, odd)), "4-byte"),
             (changed((10, off8)), "aligned"), (changed((10, off4)), "aligned"), (changed((10, odd)), "aligned"),
             (changed((9, 5), (10, off8)), "aligned"), (changed((9, 3), (10, off8)), "aligned"), (changed((9, 1), (10, off4)), "aligned"),
             (changed((9, 0), (10, off2)), "aligned"), (changed((9, 2), (10, off2)), "aligned")]
    for args, word in cases:
        assert call(*args, None) == -1, args
        msg = lib.ac_last_error().decode()
        assert "invalid argument" in msg and word in msg, (args, msg)
