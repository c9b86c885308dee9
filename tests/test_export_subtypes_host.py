"""Host side of the export subtypes (`output.wav.subtype`): the conversion of `pcm_bytes_host` against known answers derived from
its definition, `export_audio` round trips through `wav_reader`, the refusal of every other subtype, the bytes of PCM_16 and PCM_24
files pinned by hash, the configuration keys, and the subtype table and refusals of include/audiocut_hip_pack.h.  CPU only; every comparison is exact."""
import ctypes as C
import hashlib
import re
import struct

import numpy as np
import pytest

import abi_surface
from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import wav_reader as WR

SR = 44100
SUBTYPES = ("PCM_U8", "PCM_16", "PCM_24", "PCM_32", "FLOAT", "DOUBLE")
WIDTH = {"PCM_U8": 1, "PCM_16": 2, "PCM_24": 3, "PCM_32": 4, "FLOAT": 4, "DOUBLE": 8}
READER_FORMAT = {"PCM_U8": "u8", "PCM_16": "s16", "PCM_24": "s24", "PCM_32": "s32", "FLOAT": "f32", "DOUBLE": "f64"}

# the conversion's definition: s = float32(x) * 2^31 in float32; s >= 2147483647.0f -> 0x7FFFFFFF, s <= -2^31 -> -2^31, NaN -> 0,
# else s rounded half to even.  float32(0.9) = 15099494 / 2^24 and float32(0.1) = 13421773 / 2^27, so the last two products are
# 15099494 and -1677721.625 exactly.
KNOWN_X = np.array([0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, np.nan, 0.9 * 2.0 ** -7, -0.1 * 2.0 ** -7], dtype=np.float32)
KNOWN_V32 = [0, 2 ** 30, -2 ** 30, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, 15099494, -1677722]
KNOWN_U8 = [128, 192, 64, 255, 0, 255, 0, 128, 128, 127]


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------
def test_integer_subtypes_known_answers():
    got, width = AE.pcm_bytes_host(KNOWN_X, "PCM_U8")
    assert width == 1 and got.dtype == np.uint8 and got.tolist() == KNOWN_U8
    assert [(v >> 24) + 128 for v in KNOWN_V32] == KNOWN_U8
    got, width = AE.pcm_bytes_host(KNOWN_X, "PCM_32")
    assert width == 4 and got.view("<i4").tolist() == KNOWN_V32
    got, width = AE.pcm_bytes_host(KNOWN_X, "PCM_16")
    assert width == 2 and got.view("<i2").tolist() == [v >> 16 for v in KNOWN_V32]
    got, width = AE.pcm_bytes_host(KNOWN_X, "PCM_24")
    assert width == 3
    b = got.reshape(-1, 3).astype(np.int64)
    words = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    assert np.where(words & 0x800000, words - 0x1000000, words).tolist() == [v >> 8 for v in KNOWN_V32]


def test_float_subtypes_keep_the_bits():
    bits = np.array([0x00000001, 0x807FFFFF, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x3F800000, 0x00800000], dtype="<u4")
    x = bits.view("<f4")                                   # two denormals, -0.0, +-inf, a NaN with a payload, 1.0, the least normal
    got, width = AE.pcm_bytes_host(x, "FLOAT")
    assert width == 4 and got.dtype == np.uint8 and got.view("<u4").tolist() == bits.tolist()
    got, width = AE.pcm_bytes_host(x, "DOUBLE")
    assert width == 8 and got.view("<u8").tolist() == x.astype("<f8").view("<u8").tolist()
    finite = np.isfinite(x)
    assert (got.view("<f8")[finite].astype(np.float32).view("<u4") == bits[finite]).all()      # the widening is exact
    assert np.signbit(got.view("<f8")[2]) and got.view("<f8")[2] == 0.0
    got, _ = AE.pcm_bytes_host(KNOWN_X, "DOUBLE")
    assert got.view("<u8").tolist() == KNOWN_X.astype("<f8").view("<u8").tolist()


# ---- 2. round trip ------------------------------------------------------------------------------------------------------------
def _track(n: int, channels: int) -> np.ndarray:
    rng = np.random.default_rng(100 * n + channels)
    x = np.clip(0.6 * rng.standard_normal((channels, n)), -1.3, 1.3).astype(np.float32)
    x.reshape(-1)[: min(x.size, KNOWN_X.size)] = KNOWN_X[: min(x.size, KNOWN_X.size)]
    return x if channels == 2 else x[0]


def _chunks(blob: bytes, unpadded_tail: bool = False):
    """[(id, offset of the body, size)] of a RIFF/WAVE file whose chunks must tile it exactly (`unpadded_tail`: but for the pad
    byte of an odd last chunk, which PCM_24 files here have never had and still must not have)."""
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WAVE" and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8
    out, pos = [], 12
    while pos < len(blob):
        cid, size = struct.unpack("<4sI", blob[pos: pos + 8])
        out.append((cid, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == len(blob) + (1 if unpadded_tail and out[-1][2] & 1 else 0)
    return out


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 5, 4099])
@pytest.mark.parametrize("subtype", SUBTYPES)
def test_export_audio_round_trip(tmp_path, subtype, n, channels):
    x = _track(n, channels)
    path = AE.export_audio(x, SR, tmp_path / "t", "wav", options={"subtype": subtype})
    info = WR.read_wav_info(path)
    assert (info.sample_format, info.container_bytes, info.channels, info.n_frames, info.sample_rate) == \
        (READER_FORMAT[subtype], WIDTH[subtype], channels, n, SR)
    ready, width = AE.pcm_bytes_host(x.T if channels == 2 else x, subtype)
    assert width == WIDTH[subtype] and ready.size == n * channels * width
    raw = WR.read_wav_bytes(path, info)
    assert raw.tobytes() == ready.tobytes()
    got = WR.decode_samples(raw, info)
    want = WR.decode_samples(ready, info)
    assert got.shape == (n, channels) and got.view("<u4").tolist() == want.view("<u4").tolist()
    if subtype == "FLOAT":
        assert got.view("<u4").tolist() == np.ascontiguousarray(x.T if channels == 2 else x.reshape(-1, 1)).view("<u4").tolist()
    # the header: format tag, chunk order, the fact chunk of the float subtypes, the pad byte of an odd data chunk
    blob = path.read_bytes()
    chunks = _chunks(blob, unpadded_tail=subtype == "PCM_24")
    is_float = subtype in ("FLOAT", "DOUBLE")
    assert [c[0] for c in chunks] == ([b"fmt ", b"fact", b"data"] if is_float else [b"fmt ", b"data"])
    assert not any(c[0] == b"PEAK" for c in chunks)
    fmt = chunks[0]
    assert fmt[2] == 16
    tag, ch, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", blob[fmt[1]: fmt[1] + 16])
    assert (tag, ch, rate, byte_rate, align, bits) == (3 if is_float else 1, channels, SR, SR * channels * width, channels * width, 8 * width)
    if is_float:
        assert chunks[1][2] == 4 and struct.unpack("<I", blob[chunks[1][1]: chunks[1][1] + 4])[0] == n
    data = chunks[-1]
    assert data[2] == ready.size and data[1] == info.data_offset == (56 if is_float else 44)
    pad = 1 if subtype == "PCM_U8" and (n * channels) % 2 else 0
    assert (ready.size & 1) == (1 if pad or (subtype == "PCM_24" and (n * channels) % 2) else 0)
    assert len(blob) == data[1] + data[2] + pad and (not pad or blob[-1] == 0)
    assert blob[: data[1]] == AE.wav_header(n, SR, channels, width, subtype)


def test_packed_track_slices_and_from_bytes(tmp_path):
    for subtype in SUBTYPES:
        for channels in (1, 2):
            x = _track(11, channels)
            pk = AE.PackedTrack(x, SR, subtype)
            assert (pk.width, pk.channels, pk.n, pk.subtype) == (WIDTH[subtype], channels, 11, subtype)
            a = pk.write(tmp_path / "a.wav", 2, 9).read_bytes()
            piece = x[..., 2:9]
            b = AE.export_audio(piece, SR, tmp_path / "b", "wav", options={"subtype": subtype}).read_bytes()
            assert a == b
            ready, _ = AE.pcm_bytes_host(x.T if channels == 2 else x, subtype)
            again = AE.PackedTrack.from_bytes(ready.tobytes(), 11, channels, SR, subtype)
            assert again.write(tmp_path / "c.wav", 2, 9).read_bytes() == a and again.subtype == subtype
            with pytest.raises(ValueError):
                AE.PackedTrack.from_bytes(ready[:-1], 11, channels, SR, subtype)
    with pytest.raises(ValueError, match="PCM_S8"):
        AE.PackedTrack.from_bytes(b"", 0, 1, SR, "PCM_S8")


def test_header_refuses_what_does_not_fit_32_bits():
    assert len(AE.wav_header((2 ** 32 - 64) // 8, SR, 2, 4, "FLOAT")) == 56
    for args in (((2 ** 32) // 8, SR, 2, 4, "FLOAT"), (2 ** 32, SR, 1, 1, "PCM_U8"), (2 ** 31, SR, 1, 3, None), ((2 ** 32 - 8) // 8, SR, 1, 8, "DOUBLE")):
        with pytest.raises(ValueError, match="RF64"):
            AE.wav_header(*args)
    with pytest.raises(ValueError):
        AE.wav_header(4, SR, 1, 3, "PCM_16")               # a width that is not the subtype's


# ---- 3. every other subtype is refused ------------------------------------------------------------------------------------------
def test_unknown_subtype_raises(tmp_path):
    x = np.zeros(8, np.float32)
    for name in ("ULAW", "ALAW", "IMA_ADPCM", "MS_ADPCM", "PCM_S8", "pcm_24", "FLOAT32", "", None):
        with pytest.raises(ValueError) as err:
            AE.pcm_bytes_host(x, name)
        assert repr(name) in str(err.value) and all(s in str(err.value) for s in SUBTYPES)
    with pytest.raises(ValueError, match="PCM_S8"):
        AE.export_audio(x, SR, tmp_path / "x", "wav", options={"subtype": "PCM_S8"})
    assert not list(tmp_path.iterdir())
    with pytest.raises(ValueError, match="ULAW"):
        AE.PackedTrack(x, SR, "ULAW")


# ---- 4. the formats that were written before, byte for byte ------------------------------------------------------------------------
def _fixed(channels: int) -> np.ndarray:
    """Exact rationals in [-1.25, 1.25], 1001 frames: every float32 is a correctly rounded quotient, whatever the platform."""
    i = np.arange(1001 * channels, dtype=np.int64)
    x = (((i * 7919) % 2001 - 1000).astype(np.float32) / np.float32(800.0)).reshape(channels, 1001)
    return x if channels == 2 else x[0]


# sha256 of wav_header(1001, 44100, channels, width) + pcm_bytes_host(fixed track)[0] for the mono and then the stereo track, taken
# on the commit before any other subtype was written
PARENT_SHA256 = {
    "PCM_24": "d9ce2b92a27796a407ff950a6c6b1f82c9e3eec0d649680c77917f8bdd90317b",
    "PCM_16": "057a2c52aa3170d936015d6445d233d2b1e44c2bf1b5bde8f3efaf89553ebba3",
}


@pytest.mark.parametrize("subtype", ["PCM_24", "PCM_16"])
def test_pcm24_and_pcm16_files_are_unchanged(tmp_path, subtype):
    h = hashlib.sha256()
    for channels in (1, 2):
        x = _fixed(channels)
        blob = AE.export_audio(x, SR, tmp_path / f"f{channels}", "wav", options={"subtype": subtype}).read_bytes()
        ready, width = AE.pcm_bytes_host(x.T if channels == 2 else x, subtype)
        assert blob == AE.wav_header(1001, SR, channels, width) + ready.tobytes() == AE.wav_header(1001, SR, channels, width, subtype) + ready.tobytes()
        assert AE.PackedTrack(x, SR, subtype).write(tmp_path / "p.wav").read_bytes() == blob
        h.update(blob)
    assert h.hexdigest() == PARENT_SHA256[subtype]
    if subtype == "PCM_24":                                 # the default is still PCM_24
        assert AE.export_audio(_fixed(1), SR, tmp_path / "d", "wav").read_bytes() == \
            AE.export_audio(_fixed(1), SR, tmp_path / "e", "wav", options={"subtype": "PCM_24"}).read_bytes()


# ---- configuration --------------------------------------------------------------------------------------------------------------
def test_configuration_keys():
    from audio_cut_amd import config
    assert config.DEFAULTS["output"] == {"format": "wav", "wav": {"subtype": "PCM_24"}}
    saved = config.snapshot()
    try:
        assert AE.configured_subtype() == "PCM_24"
        config.set_runtime_config({"output.wav.subtype": "PCM_16"})
        assert AE.configured_subtype() == "PCM_16"
        config.set_runtime_config({"output.wav.subtype": "ULAW"})
        with pytest.raises(ValueError, match="ULAW"):
            AE.configured_subtype()
        config.set_runtime_config({"output.wav.subtype": "FLOAT", "output.format": "mp3"})
        with pytest.raises(ValueError) as err:
            AE.configured_subtype()
        with pytest.raises(ValueError) as want:
            AE.ensure_supported_format("mp3")
        assert str(err.value) == str(want.value)
    finally:
        config.restore(saved)
    assert AE.configured_subtype() == "PCM_24"


def test_api_refuses_the_format_before_any_work(tmp_path):
    """`separate_and_segment(runtime_overrides={"output.format": "mp3"})` raises as `ensure_supported_format("mp3")` does, and an
    unknown subtype raises too: both before the track is loaded (no device is needed to get there), and the configuration is
    put back."""
    import wave
    from audio_cut_amd import api, config
    src = tmp_path / "in.wav"
    with wave.open(str(src), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(np.zeros(64, "<i2").tobytes())
    with pytest.raises(ValueError) as want:
        AE.ensure_supported_format("mp3")
    for overrides, message in (({"output.format": "mp3"}, str(want.value)), ({"output.wav.subtype": "ULAW"}, "'ULAW'")):
        with pytest.raises(ValueError) as err:
            api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), runtime_overrides=overrides)
        assert message in str(err.value)
        assert config.get_config("output.format") == "wav" and config.get_config("output.wav.subtype") == "PCM_24"
    assert not list((tmp_path / "out").iterdir())


# ---- include/audiocut_hip_pack.h --------------------------------------------------------------------------------------------------
def test_subtype_table_is_the_headers_the_librarys_and_the_hosts(lib):
    from audio_cut_amd import _native
    codes = dict(re.findall(r"#define AC_PACK_(PCM_U8|PCM_16|PCM_24|PCM_32|FLOAT|DOUBLE) (\d)", abi_surface.code("audiocut_hip_pack.h")))
    assert {k: (int(v), WIDTH[k]) for k, v in codes.items()} == AE.WAV_SUBTYPES == _native.PACK_SUBTYPES
    for name, (code, width) in AE.WAV_SUBTYPES.items():
        assert lib.ac_pack_width(code) == width
        assert lib.ac_pack_out_align(code) == {1: 4, 2: 8, 3: 4, 4: 16, 8: 16}[width]
    assert lib.ac_pack_width(6) == lib.ac_pack_width(-1) == lib.ac_pack_out_align(6) == 0


def test_pack_entry_points_reject_bad_arguments(lib):
    """Every refusal comes back as AC_E_INVALID with a message, before anything is launched.  The context handle is never read by
    the checks, so a placeholder stands in for one here (no device on this machine)."""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    raw = C.create_string_buffer(256)
    addr = (C.addressof(raw) + 15) & ~15
    buf, odd, off2, off4, off8 = (C.c_void_p(addr + k) for k in (0, 1, 2, 4, 8))
    call = lib.ac_pack_pcm
    good = [buf, 8, 2, 8, 4, buf]                        # x, n_frames, channels, row_stride, subtype, out
    cases = [([None] + good, "null")]
    def changed(index, value, base=good):
        args = list(base)
        args[index] = value
        return [ctx] + args
    cases += [(changed(0, None), "null"), (changed(5, None), "null"), (changed(1, 0), "n_frames"), (changed(1, -1), "n_frames"),
              (changed(1, 2 ** 40), "too long"), (changed(2, 0), "channels"), (changed(2, 3), "channels"), (changed(3, 7), "row_stride"),
              (changed(4, 6), "subtype"), (changed(4, -1), "subtype"), (changed(0, off2), "4-byte"), (changed(0, odd), "4-byte"),
              (changed(5, off8), "aligned"), (changed(5, off4), "aligned"), (changed(5, odd), "aligned"),
              (changed(5, off8, changed(4, 5)[1:]), "aligned"), (changed(5, off4, changed(4, 1)[1:]), "aligned"),
              (changed(5, off2, changed(4, 0)[1:]), "aligned"), (changed(5, off2, changed(4, 2)[1:]), "aligned")]
    for args, word in cases:
        assert call(*args, None) == -1, args
        assert word in lib.ac_last_error().decode(), (args, lib.ac_last_error())

    call = lib.ac_mdx_assemble_pcm
    good = [buf, 8, 1, buf, buf, buf, buf, buf, buf, 1, 3, buf, buf, buf, 1]   # as ac_mdx_assemble_pcm24, the subtype behind n_chunks
    assert call(None, *good, None) == -1 and "null" in lib.ac_last_error().decode()
    cases = [(changed(i, None, good), "null") for i in (0, 3, 4, 5, 6, 7, 8, 11, 12, 13)]
    cases += [(changed(1, 0, good), "sizes"), (changed(9, 0, good), "sizes"), (changed(2, 3, good), "channels"),
              (changed(10, 6, good), "subtype"), (changed(10, -1, good), "subtype"),
              (changed(11, off4, good), "aligned"), (changed(12, off8, good), "aligned"), (changed(0, off4, good), "aligned"),
              (changed(11, off4, changed(10, 1, good)[1:]), "aligned"), (changed(12, off2, changed(10, 2, good)[1:]), "aligned"),
              (changed(14, 0, good), "n_partials"), (changed(14, 4097, good), "n_partials")]
    for args, word in cases:
        assert call(*args, None) == -1, args
        assert word in lib.ac_last_error().decode(), (args, lib.ac_last_error())
