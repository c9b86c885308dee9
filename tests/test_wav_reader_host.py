"""The RIFF/WAVE reader (audio_cut_amd/utils/wav_reader.py), the host loaders built on it, and the constants and refusals
of include/audiocut_hip_load.h.  CPU only: files are built with `struct`, every comparison is exact."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import abi_surface
from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd.utils import wav_reader as WR
from audio_cut_amd.utils.wav_reader import UnsupportedAudioError

KS_TAIL = bytes.fromhex("000000001000800000AA00389B71")


def chunk(cid: bytes, body: bytes, size=None) -> bytes:
    """One RIFF chunk; an odd body gets its pad byte.  `size` overrides the length field (the body is written as given)."""
    n = len(body) if size is None else size
    return cid + struct.pack("<I", n) + body + (b"\0" if size is None and len(body) & 1 else b"")


def fmt_body(tag, channels, rate, width, bits=None, size=16, sub_tag=None, valid=None, tail=KS_TAIL, block_align=None):
    bits = 8 * width if bits is None else bits
    ba = channels * width if block_align is None else block_align
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * ba, ba, bits)
    if size == 18:
        body += struct.pack("<H", 0)
    if size == 40:
        body += struct.pack("<HHI", 22, bits if valid is None else valid, 0) + struct.pack("<H", sub_tag) + tail
    return body


def riff(*chunks, magic=b"RIFF") -> bytes:
    payload = b"WAVE" + b"".join(chunks)
    return magic + struct.pack("<I", len(payload)) + payload


def write(tmp_path, name, blob) -> Path:
    p = tmp_path / name
    p.write_bytes(blob)
    return p


PCM = bytes(range(1, 49))                      # 48 bytes: 12 stereo s16 frames, 8 stereo s24 frames, 6 stereo s32 frames


# ---- headers -----------------------------------------------------------------------------------------------------------------------

def test_plain_16_and_18_byte_fmt(tmp_path):
    for size in (16, 18):
        p = write(tmp_path, f"p{size}.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2, size=size)), chunk(b"data", PCM)))
        info = WR.read_wav_info(p)
        assert info == WR.WavInfo(sample_rate=44100, channels=2, sample_format="s16", container_bytes=2, bits_per_sample=16,
                                  n_frames=12, data_offset=12 + 8 + size + 8, data_bytes=48)
        assert info.format_code == 1
        assert WR.read_wav_bytes(p, info).tobytes() == PCM


def test_extensible_pcm_and_float(tmp_path):
    p = write(tmp_path, "x24.wav", riff(chunk(b"fmt ", fmt_body(0xFFFE, 2, 48000, 3, size=40, sub_tag=1)), chunk(b"data", PCM)))
    info = WR.read_wav_info(p)
    assert (info.sample_rate, info.channels, info.sample_format, info.container_bytes, info.bits_per_sample, info.n_frames) == \
        (48000, 2, "s24", 3, 24, 8)
    p = write(tmp_path, "xf32.wav", riff(chunk(b"fmt ", fmt_body(0xFFFE, 6, 48000, 4, size=40, sub_tag=3)), chunk(b"data", PCM)))
    info = WR.read_wav_info(p)
    assert (info.channels, info.sample_format, info.container_bytes, info.n_frames, info.data_bytes) == (6, "f32", 4, 2, 48)
    p = write(tmp_path, "f64.wav", riff(chunk(b"fmt ", fmt_body(3, 1, 8000, 8, size=18)), chunk(b"fact", struct.pack("<I", 6)),
                                        chunk(b"data", PCM)))
    assert (WR.read_wav_info(p).sample_format, WR.read_wav_info(p).n_frames) == ("f64", 6)
    p = write(tmp_path, "u8.wav", riff(chunk(b"fmt ", fmt_body(1, 1, 8000, 1)), chunk(b"data", PCM)))
    assert (WR.read_wav_info(p).sample_format, WR.read_wav_info(p).n_frames) == ("u8", 48)


def test_chunks_around_data_are_skipped_with_their_pad_byte(tmp_path):
    odd_list = chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 5) + b"abcd\0")         # 17 bytes: padded to 18
    assert len(odd_list) == 8 + 17 + 1
    blob = riff(chunk(b"JUNK", bytes(28)), chunk(b"fmt ", fmt_body(1, 2, 44100, 2)), chunk(b"bext", bytes(7)), odd_list,
                chunk(b"data", PCM), chunk(b"LIST", b"adtl" + bytes(9)), chunk(b"id3 ", bytes(3)))
    p = write(tmp_path, "chunks.wav", blob)
    info = WR.read_wav_info(p)
    assert info.n_frames == 12 and blob[info.data_offset: info.data_offset + info.data_bytes] == PCM
    # a pad byte that is ignored would put the walk one byte off and lose the data chunk
    assert WR.read_wav_bytes(p, info).tobytes() == PCM


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF, 1000])
def test_data_length_of_a_writer_that_could_not_seek_back(tmp_path, size):
    p = write(tmp_path, "pipe.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2)), chunk(b"data", PCM, size=size)))
    info = WR.read_wav_info(p)
    assert (info.n_frames, info.data_bytes) == (12, 48) and WR.read_wav_bytes(p, info).tobytes() == PCM


def test_trailing_partial_frame_is_dropped_and_no_frame_is_an_error(tmp_path):
    p = write(tmp_path, "part.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 3)), chunk(b"data", PCM[:47])))
    info = WR.read_wav_info(p)
    assert (info.n_frames, info.data_bytes) == (7, 42) and WR.read_wav_bytes(p, info).tobytes() == PCM[:42]
    p = write(tmp_path, "empty.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 3)), chunk(b"data", PCM[:5])))
    with pytest.raises(ValueError, match="no whole frame"):
        WR.read_wav_info(p)
    p = write(tmp_path, "empty2.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2)), chunk(b"data", b"")))
    with pytest.raises(ValueError, match="no whole frame"):
        WR.read_wav_info(p)


def test_24_valid_bits_in_a_4_byte_container_is_a_32_bit_file(tmp_path):
    raw = struct.pack("<4i", 0x12345600, -0x12345600, 0x7FFFFF00, -0x80000000)
    want = np.array([0x12345600, -0x12345600, 0x7FFFFF00, -0x80000000], dtype=np.int64).astype(np.float32) / np.float32(2.0 ** 31)
    for name, body in (("plain", fmt_body(1, 1, 44100, 4, bits=24)), ("ext", fmt_body(0xFFFE, 1, 44100, 4, bits=32, valid=24, size=40, sub_tag=1))):
        p = write(tmp_path, f"24in32_{name}.wav", riff(chunk(b"fmt ", body), chunk(b"data", raw)))
        info = WR.read_wav_info(p)
        assert (info.sample_format, info.container_bytes, info.bits_per_sample, info.n_frames) == ("s32", 4, 24, 4)
        got = WR.decode_host(WR.read_wav_bytes(p, info), info, WR.LAYOUT_MONO)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert got[0] == np.float32(0x123456 / 2.0 ** 23)                   # left-justified: the 24 bits are the top three bytes


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def _refusal_cases():
    ok_fmt, data = chunk(b"fmt ", fmt_body(1, 2, 44100, 2)), chunk(b"data", PCM)
    bad_guid = KS_TAIL[:-1] + b"\x72"
    return [
        ("rf64", riff(ok_fmt, data, magic=b"RF64"), "RF64"),
        ("rifx", riff(ok_fmt, data, magic=b"RIFX"), "RIFX"),
        ("not_riff", b"FORM" + bytes(40), "not a RIFF/WAVE"),
        ("not_wave", b"RIFF" + struct.pack("<I", 40) + b"AVI " + bytes(36), "not a RIFF/WAVE"),
        ("alaw", riff(chunk(b"fmt ", fmt_body(6, 1, 8000, 1, size=18)), data), "A-law"),
        ("mulaw", riff(chunk(b"fmt ", fmt_body(7, 1, 8000, 1, size=18)), data), "mu-law"),
        ("adpcm", riff(chunk(b"fmt ", fmt_body(2, 2, 44100, 2, size=18)), data), "ADPCM"),
        ("ima", riff(chunk(b"fmt ", fmt_body(0x11, 2, 44100, 2, size=18)), data), "ADPCM"),
        ("mpeg", riff(chunk(b"fmt ", fmt_body(0x55, 2, 44100, 2, size=18)), data), "MPEG"),
        ("other_tag", riff(chunk(b"fmt ", fmt_body(0x1234, 2, 44100, 2)), data), "format tag 0x1234"),
        ("ext_alaw", riff(chunk(b"fmt ", fmt_body(0xFFFE, 1, 8000, 1, size=40, sub_tag=6)), data), "A-law"),
        ("guid", riff(chunk(b"fmt ", fmt_body(0xFFFE, 2, 44100, 2, size=40, sub_tag=1, tail=bad_guid)), data), "GUID mismatch"),
        ("ext_short", riff(chunk(b"fmt ", fmt_body(0xFFFE, 2, 44100, 2, size=18)), data), "40-byte fmt"),
        ("fmt_size", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2) + bytes(4)), data), "fmt chunk of 20 bytes"),
        ("block_align", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2, block_align=5)), data), "inconsistent block_align"),
        ("block_align_width", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 5)), data), "inconsistent block_align"),
        ("bits_over_width", riff(chunk(b"fmt ", fmt_body(1, 2, 44100, 2, bits=24)), data), "inconsistent block_align"),
        ("float16", riff(chunk(b"fmt ", fmt_body(3, 2, 44100, 2)), data), "inconsistent block_align"),
        ("channels0", riff(chunk(b"fmt ", fmt_body(1, 0, 44100, 2)), data), "0 channels"),
        ("channels9", riff(chunk(b"fmt ", fmt_body(1, 9, 44100, 2)), data), "9 channels"),
        ("no_fmt", riff(chunk(b"LIST", bytes(6)), data), "no fmt chunk"),
        ("no_data", riff(ok_fmt, chunk(b"LIST", bytes(6))), "no data chunk"),
    ]


@pytest.mark.parametrize("name,blob,cause", _refusal_cases(), ids=[c[0] for c in _refusal_cases()])
def test_refusals_name_their_cause(tmp_path, name, blob, cause):
    p = write(tmp_path, name + ".wav", blob)
    with pytest.raises(UnsupportedAudioError) as err:
        WR.read_wav_info(p)
    assert cause in str(err.value) and str(p) in str(err.value)
    assert isinstance(err.value, ValueError)
    from audio_cut_amd import api
    with pytest.raises(UnsupportedAudioError):
        api.load_audio_mono(str(p))


# ---- decode_host -------------------------------------------------------------------------------------------------------------------

def _info(fmt, channels, n):
    w = WR.SAMPLE_FORMATS[fmt][1]
    return WR.WavInfo(sample_rate=44100, channels=channels, sample_format=fmt, container_bytes=w, bits_per_sample=8 * w, n_frames=n,
                      data_offset=44, data_bytes=n * channels * w)


def _mono(fmt, raw):
    raw = np.frombuffer(raw, dtype=np.uint8)
    out = WR.decode_host(raw, _info(fmt, 1, raw.size // WR.SAMPLE_FORMATS[fmt][1]), WR.LAYOUT_MONO)
    assert out.dtype == np.float32
    return out


def test_decode_known_answers():
    f = np.float32
    assert np.array_equal(_mono("u8", bytes([0, 1, 127, 128, 129, 255])), np.array([-1.0, -127 / 128, -1 / 128, 0.0, 1 / 128, 127 / 128], f))
    assert np.array_equal(_mono("s16", struct.pack("<6h", -32768, -1, 0, 1, 32767, 16384)),
                          np.array([-1.0, -2.0 ** -15, 0.0, 2.0 ** -15, 32767 / 32768, 0.5], f))
    s24 = b"\x00\x00\x80" + b"\xff\xff\xff" + b"\x00\x00\x00" + b"\x01\x00\x00" + b"\xff\xff\x7f" + b"\x56\x34\x12"
    assert np.array_equal(_mono("s24", s24), np.array([-1.0, -2.0 ** -23, 0.0, 2.0 ** -23, 8388607 / 8388608, 0x123456 / 2.0 ** 23], f))
    # s32: 2^31 - 1 and 2^24 + 1 are no float32; ties go to the even mantissa (2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4)
    s32 = struct.pack("<8i", -2 ** 31, -1, 0, 1, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1))
    assert np.array_equal(_mono("s32", s32), np.array([-1.0, -2.0 ** -31, 0.0, 2.0 ** -31, 1.0, 2.0 ** -7, (2 ** 24 + 4) / 2.0 ** 31, -2.0 ** -7], f))
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -3.25, 1e-45, 3.4e38], f)               # beyond +-1, a denormal: nothing is clipped
    got = _mono("f32", vals.tobytes())
    assert np.array_equal(got.view(np.uint32), vals.view(np.uint32))
    d = np.array([0.0, -0.0, 1.0, -2.5, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 0.1, 1e300, -1e39, 3.4028235e38], np.float64)
    want = np.array([0.0, -0.0, 1.0, -2.5, 1.0, 1.0 + 2.0 ** -22, f(0.1), np.inf, -np.inf, 3.4028235e38], f)   # ties to even; overflow
    got = _mono("f64", d.tobytes())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    raw = np.frombuffer(d.tobytes(), dtype=np.uint8)
    assert WR.count_nonfinite(raw, _info("f64", 1, d.size)) == 2 and WR.count_nonfinite(raw[:16], _info("s16", 1, 8)) == 0
    nan32 = np.array([np.nan, np.inf, -np.inf, 1.0], f)
    assert WR.count_nonfinite(np.frombuffer(nan32.tobytes(), np.uint8), _info("f32", 2, 2)) == 3


def test_integer_formats_keep_the_first_loader_s_arithmetic():
    """The formulas of the `wave`-based loader this reader replaces, written out."""
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=24 * 999, dtype=np.uint8)
    for ch in (1, 2):
        old16 = (np.frombuffer(raw.tobytes(), dtype="<i2").astype(np.float32) / 32768.0).reshape(-1, ch)
        b = np.frombuffer(raw.tobytes(), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        old24 = (v.astype(np.float32) / 8388608.0).reshape(-1, ch)
        old32 = (np.frombuffer(raw.tobytes(), dtype="<i4").astype(np.float32) / 2147483648.0).reshape(-1, ch)
        for fmt, old in (("s16", old16), ("s24", old24), ("s32", old32)):
            info = _info(fmt, ch, old.shape[0])
            assert np.array_equal(WR.decode_host(raw, info, WR.LAYOUT_PLANAR), old.T), (fmt, ch)
            old_mono = np.mean(old, axis=1).astype(np.float32) if ch > 1 else old[:, 0].copy()
            got = WR.decode_host(raw, info, WR.LAYOUT_MONO)
            assert got.dtype == np.float32 and np.array_equal(got, old_mono), (fmt, ch)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_mono_mean_is_numpy_s_mean_over_the_channel_axis(channels):
    rng = np.random.default_rng(channels)
    x = (rng.standard_normal((5001, channels)) * np.exp(rng.uniform(-12, 3, size=(5001, channels)))).astype(np.float32)
    info = _info("f32", channels, x.shape[0])
    raw = np.frombuffer(x.tobytes(), dtype=np.uint8)
    got = WR.decode_host(raw, info, WR.LAYOUT_MONO)
    assert got.shape == (5001,) and np.array_equal(got, np.mean(x, axis=1))
    acc = x[:, 0].copy()
    for c in range(1, channels):
        acc = acc + x[:, c]
    assert np.array_equal(got, acc / np.float32(channels) if channels > 1 else acc)
    planar = WR.decode_host(raw, info, WR.LAYOUT_PLANAR)
    assert planar.shape == (channels, 5001) and planar.flags.c_contiguous and np.array_equal(planar, x.T)


# ---- host loaders ------------------------------------------------------------------------------------------------------------------

def test_host_loaders_read_plain_extensible_and_float_files(tmp_path):
    from audio_cut_amd import api
    rng = np.random.default_rng(11)
    pcm = rng.integers(-32768, 32768, size=(3001, 2), dtype=np.int16)
    data = chunk(b"data", pcm.astype("<i2").tobytes())
    plain = write(tmp_path, "plain.wav", riff(chunk(b"fmt ", fmt_body(1, 2, 48000, 2)), data))
    ext = write(tmp_path, "ext.wav", riff(chunk(b"fmt ", fmt_body(0xFFFE, 2, 48000, 2, size=40, sub_tag=1)),
                                          chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 3) + b"ab\0"), data))
    flt = write(tmp_path, "float.wav", riff(chunk(b"fmt ", fmt_body(3, 2, 48000, 4, size=18)), chunk(b"fact", struct.pack("<I", 3001)),
                                            chunk(b"data", (pcm.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes())))
    want = pcm.astype(np.float32) / 32768.0
    for p in (plain, ext, flt):
        mono, sr = api.load_audio_mono(str(p))
        st, sr2 = api.load_audio_stereo(str(p))
        assert sr == sr2 == 48000 and mono.dtype == st.dtype == np.float32
        assert np.array_equal(mono, np.mean(want, axis=1)) and np.array_equal(st, want.T) and st.flags.c_contiguous
    # float samples beyond +-1 pass; a NaN is refused with its count
    loud = np.array([[1.5, -2.0], [0.25, 3.0]], np.float32)
    p = write(tmp_path, "loud.wav", riff(chunk(b"fmt ", fmt_body(3, 2, 44100, 4)), chunk(b"data", loud.tobytes())))
    assert np.array_equal(api.load_audio_stereo(str(p))[0], loud.T)
    loud[1, 0] = np.nan
    p = write(tmp_path, "nan.wav", riff(chunk(b"fmt ", fmt_body(3, 2, 44100, 4)), chunk(b"data", loud.tobytes())))
    with pytest.raises(ValueError, match="1 samples are NaN or infinite"):
        api.load_audio_mono(str(p))
    # 8-bit PCM and a 6-channel extensible file
    p = write(tmp_path, "u8.wav", riff(chunk(b"fmt ", fmt_body(1, 1, 8000, 1)), chunk(b"data", bytes([0, 128, 255]))))
    assert np.array_equal(api.load_audio_mono(str(p))[0], np.array([-1.0, 0.0, 127 / 128], np.float32))
    six = rng.integers(-32768, 32768, size=(50, 6), dtype=np.int16)
    p = write(tmp_path, "six.wav", riff(chunk(b"fmt ", fmt_body(0xFFFE, 6, 48000, 2, size=40, sub_tag=1)), chunk(b"data", six.astype("<i2").tobytes())))
    assert np.array_equal(api.load_audio_mono(str(p))[0], np.mean(six.astype(np.float32) / 32768.0, axis=1))
    with pytest.raises(ValueError, match="6 channels; audio.channels: 2 takes mono or stereo input"):
        api.load_audio_stereo(str(p))
    assert "load_audio_device" in api.__all__
    from audio_cut_amd import config
    assert config.get_config("audio.gpu_decode") is True and config.get_config("audio.channels") == 1


def test_manifest_duration_comes_from_the_reader(tmp_path):
    from audio_cut_amd import api
    p = write(tmp_path, "x.wav", riff(chunk(b"fmt ", fmt_body(0xFFFE, 2, 48000, 3, size=40, sub_tag=1)), chunk(b"data", bytes(6 * 24000))))
    assert api._track_seconds({}, p) == 0.5
    assert api._track_seconds({"segment_durations": [1.0, 2.0]}, tmp_path / "missing.wav") == 3.0


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------

def test_load_header_constants_and_the_readers_tables_are_one_numbering():
    consts = dict(re.findall(r"#define\s+(AC_LOAD_[A-Z0-9_]+)\s+(\d+)", abi_surface.code("audiocut_hip_load.h")))
    assert {k: WR.SAMPLE_FORMATS[k][0] for k in WR.SAMPLE_FORMATS} == {k.split("_")[-1].lower(): int(v) for k, v in consts.items()
                                                                      if k.split("_")[-1].lower() in WR.SAMPLE_FORMATS}
    assert (int(consts["AC_LOAD_MONO"]), int(consts["AC_LOAD_PLANAR"])) == (WR.LAYOUT_MONO, WR.LAYOUT_PLANAR)
    assert int(consts["AC_LOAD_MAX_CHANNELS"]) == WR.MAX_CHANNELS


def test_decode_entry_refuses_before_anything_is_launched(lib):
    """AC_E_INVALID with a message for each precondition; the checks never read the context or the buffers, so placeholders stand
    in for them here (no device on this machine)."""
    mem = C.create_string_buffer(64 + 16)
    base = (C.addressof(mem) + 15) & ~15                               # a 16-byte aligned placeholder
    ok = dict(ctx=base, bytes=base, n=100, ch=2, fmt=1, layout=0, out=base, stride=100, cnt=base)
    cases = [({"ctx": None}, "null pointer"), ({"bytes": None}, "null pointer"), ({"out": None}, "null pointer"), ({"cnt": None}, "null pointer"),
             ({"n": 0}, "n_frames"), ({"n": -4}, "n_frames"), ({"ch": 0}, "channels"), ({"ch": 9}, "channels"),
             ({"fmt": -1}, "unknown sample format"), ({"fmt": 6}, "unknown sample format"),
             ({"layout": 2}, "unknown layout"), ({"layout": -1}, "unknown layout"),
             ({"bytes": base + 1}, "4-byte aligned"), ({"bytes": base + 2}, "4-byte aligned"), ({"out": base + 2}, "aligned"),
             ({"cnt": base + 4}, "aligned"),
             ({"layout": 1, "stride": 99}, "out_stride"), ({"layout": 1, "stride": 0}, "out_stride"),
             ({"n": 1 << 41}, "too long"), ({"n": (1 << 62), "layout": 1, "stride": 1 << 62}, "too long")]
    for change, word in cases:
        a = {**ok, **change}
        rc = lib.ac_decode_pcm(a["ctx"], a["bytes"], a["n"], a["ch"], a["fmt"], a["layout"], a["out"], a["stride"], a["cnt"], None)
        assert rc == -1, change
        msg = lib.ac_last_error().decode()
        assert "invalid argument" in msg and word in msg, (change, msg)
