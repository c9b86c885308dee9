"""FLAC export on the host: the known answers of the stream specification (include/flac/audiocut_flac.h), the round trip of
`flac_encode_host` through the independent decoder of tests/flac_decode.py, the size conditions, the MD5 switch, the three
settings' refusals, the unchanged WAV defaults, and the C ABI of libaudiocut_flac.so against its header.  CPU only."""
import ctypes as C
import hashlib
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_surface as A
from flac_decode import FlacError, flac_decode
from flac_signals import COUNTS, SR, signals
from audio_cut_amd import _native, config
from audio_cut_amd.utils import audio_export as AE

HEADER = "flac/audiocut_flac.h"
FLAC_CSRC = A.CSRC / "flac"
SUBTYPES = (("PCM_16", 2), ("PCM_24", 3))

KNOWN_FILE = bytes.fromhex(
    "66 4c 61 43 80 00 00 22 10 00 10 00 00 00 0b 00 00 0b 0a c4 40 f0 00 00 10 00"
    "00 00 00 00 00 00 00 00 00 00 00 00 00 00 00 00 ff f8 c9 08 00 95 00 00 00 21 bd")


@pytest.fixture(scope="module")
def FX():
    from audio_cut_amd.utils import flac_export
    return flac_export


def _pcm(x: np.ndarray, subtype: str):
    """float32 [n] or [n, 2] (frames of L, R) -> (interleaved PCM bytes, width), the project's pinned conversion."""
    return AE.pcm_bytes_host(np.asarray(x, dtype=np.float32).reshape(-1), subtype)


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_crc_known_answers(FX):
    assert FX.crc8(b"123456789") == 0xF4
    assert FX.crc16(b"123456789") == 0xFEE8


def test_the_53_byte_file(FX):
    assert len(KNOWN_FILE) == 53
    (got,) = FX.flac_encode_host(bytes(2 * 4096), 4096, 1, 2, 44100, [(0, 4096)], 4096)
    assert got == KNOWN_FILE
    samples, info = flac_decode(got)
    assert samples.shape == (4096, 1) and not samples.any() and info["md5"] == bytes(16)


def test_the_decoder_refuses_damage(FX):
    pcm, w = _pcm(0.5 * np.sin(np.arange(300) / 7.0), "PCM_16")
    (good,) = FX.flac_encode_host(pcm, 300, 1, w, SR, [(0, 300)], 256)
    flac_decode(good)
    for at in (0, 9, 20, 43, 47, len(good) // 2, len(good) - 1):       # marker, STREAMINFO, sync, header, body, CRC-16
        bad = bytearray(good)
        bad[at] ^= 0x10
        with pytest.raises(FlacError):
            flac_decode(bytes(bad))


# ---- round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_size", (256, 4096))
@pytest.mark.parametrize("subtype,width", SUBTYPES)
@pytest.mark.parametrize("channels", (1, 2))
def test_round_trip(FX, channels, subtype, width, block_size):
    kinds = set()
    for n in COUNTS:
        for name, x in signals(n, channels):
            pcm, w = _pcm(x, subtype)
            assert w == width
            (data,) = FX.flac_encode_host(pcm, n, channels, width, SR, [(0, n)], block_size)
            got, info = flac_decode(data)
            want = FX.pcm_words(pcm, n, channels, width)
            assert got.shape == want.shape and (got == want).all(), (n, name)
            assert (info["sample_rate"], info["channels"], info["bits"], info["total"]) == (SR, channels, 8 * width, n)
            assert info["frames"] == -(-n // block_size)
            assert len(data) <= 42 + pcm.size + 20 * info["frames"], (n, name)             # never larger than verbatim coding
            if n == COUNTS[-1]:
                kinds |= _subframe_kinds(data, info, channels)
    # the signals reach what they are there for
    assert {"constant", "verbatim", "fixed", "method0"} <= kinds
    if width == 3:
        assert "method1" in kinds
    if channels == 2:
        assert {1, 8, 10} <= kinds or {1, 9, 10} <= kinds


def _subframe_kinds(data: bytes, info, channels: int) -> set:
    """What the frames of a file use: subframe types of the first subframe, Rice methods, channel assignments (read from the bytes)."""
    kinds, at = set(), 42
    for size in info["frame_sizes"]:
        head = data[at: at + 16]
        number_bytes = 1 if head[4] < 0x80 else 2 if head[4] >> 5 == 6 else 3 if head[4] >> 4 == 14 else 4
        extra = {6: 1, 7: 2}.get(head[2] >> 4, 0)
        first = data[at + 4 + number_bytes + extra + 1]
        kind = (first >> 1) & 0x3F
        kinds.add("constant" if kind == 0 else "verbatim" if kind == 1 else "fixed")
        if channels == 2:
            kinds.add(head[3] >> 4)
        if kind >= 8:
            order = kind - 8
            bps = info["bits"] + (1 if (head[3] >> 4) == 9 else 0)
            bit = 8 + order * bps                                           # the two method bits behind the warm-up samples
            byte = data[at + 4 + number_bytes + extra + 1 + bit // 8: at + 4 + number_bytes + extra + 3 + bit // 8]
            method = (int.from_bytes(byte, "big") >> (14 - bit % 8)) & 3
            kinds.add(f"method{method}")
        at += size
    return kinds


@pytest.mark.parametrize("frames", (130, 2050))
def test_frame_number_code_boundaries(FX, frames):
    """Silence at block 256: the frame number grows from one byte to two (at 128) and from two to three (at 2048)."""
    n = 256 * frames
    (data,) = FX.flac_encode_host(bytes(2 * n), n, 1, 2, SR, [(0, n)], 256)
    got, info = flac_decode(data)
    assert got.shape == (n, 1) and not got.any() and info["frames"] == frames
    want = [4 + (1 if f < 128 else 2 if f < 2048 else 3) + 1 + 3 + 2 for f in range(frames)]
    assert info["frame_sizes"] == want
    assert len(data) == 42 + sum(want)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subtype,width", SUBTYPES)
def test_silent_file_size_is_exact(FX, subtype, width):
    """header bytes + one subframe byte + the value + CRC-16 per frame: 11 bytes per full frame at PCM_16."""
    for n, block in ((4096, 4096), (3 * 4096 + 5, 4096), (700, 256), (100, 512)):
        (data,) = FX.flac_encode_host(bytes(width * n), n, 1, width, SR, [(0, n)], block)
        full, last = divmod(n, block)
        header = lambda f, short: 4 + (1 if f < 128 else 2) + (0 if not short else 1 if short - 1 < 256 else 2) + 1
        want = 42 + sum(header(f, 0) + 3 + width for f in range(full)) + (header(full, last) + 3 + width if last else 0)
        assert len(data) == want
        if width == 2 and not last:
            assert len(data) == 42 + 11 * full


@pytest.mark.parametrize("subtype,width", SUBTYPES)
def test_a_sine_is_under_half_its_pcm(FX, subtype, width):
    """An exhaustive single-partition estimate gives 0.23 (PCM_16) and 0.33 (PCM_24) of the PCM bytes for this second of sine."""
    x = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(SR) / SR)
    pcm, _ = _pcm(x, subtype)
    (data,) = FX.flac_encode_host(pcm, SR, 1, width, SR, [(0, SR)], 4096)
    ratio = len(data) / pcm.size
    print(f"{subtype}: {len(data)} bytes, {ratio:.3f} of the PCM bytes")
    assert ratio < 0.5
    got, _ = flac_decode(data)
    assert (got == FX.pcm_words(pcm, SR, 1, width)).all()


# ---- spans, MD5, refusals ---------------------------------------------------------------------------------------------------------
def test_spans_are_independent_files_and_md5(FX):
    rng = np.random.default_rng(3)
    n = 9000
    x = np.stack([0.4 * np.sin(np.arange(n) / 9.0), rng.uniform(-0.5, 0.5, n)], axis=1)
    pcm, w = _pcm(x, "PCM_24")
    spans = [(0, n), (17, 4113), (4000, 4001), (4000, 4002), (100, 8999)]           # overlapping, 1 and 2 samples
    plain = FX.flac_encode_host(pcm, n, 2, w, 48000, spans, 1024)
    signed = FX.flac_encode_host(pcm, n, 2, w, 48000, spans, 1024, md5=True)
    words = FX.pcm_words(pcm, n, 2, w)
    for (lo, hi), a, b in zip(spans, plain, signed):
        assert a[26:42] == bytes(16)
        assert b[26:42] == hashlib.md5(pcm[lo * 2 * w: hi * 2 * w].tobytes()).digest()
        assert a[:26] == b[:26] and a[42:] == b[42:]
        got, info = flac_decode(b)
        assert (got == words[lo:hi]).all() and info["sample_rate"] == 48000
        assert a == FX.flac_encode_host(pcm[lo * 2 * w: hi * 2 * w], hi - lo, 2, w, 48000, [(0, hi - lo)], 1024)[0]
    table = FX.frame_table(spans, 1024)
    assert table.shape == (9 + 4 + 1 + 1 + 9, 4) and table[9].tolist() == [1, 0, 17, 1024] and table[12].tolist() == [1, 3, 17 + 3072, 1024]
    assert table[8].tolist() == [0, 8, 8192, 808]


def test_refusals_by_name(FX):
    pcm = bytes(6 * 100)
    for spans in ([], [(5, 5)], [(-1, 4)], [(0, 101)], [(7, 3)]):
        with pytest.raises(ValueError):
            FX.flac_encode_host(pcm, 100, 2, 3, SR, spans, 4096)
    with pytest.raises(ValueError, match="4000"):
        FX.flac_encode_host(pcm, 100, 2, 3, SR, [(0, 100)], 4000)
    with pytest.raises(ValueError, match="2000000"):
        FX.flac_encode_host(pcm, 100, 2, 3, 2_000_000, [(0, 100)], 4096)
    with pytest.raises(ValueError, match="2000000"):
        FX.flac_header(2_000_000, 1, 16, 10, 4096, 11, 11)
    with pytest.raises(ValueError):
        FX.flac_encode_host(pcm, 100, 2, 4, SR, [(0, 100)], 4096)                  # 32-bit words
    with pytest.raises(ValueError, match="frames"):
        FX.frame_table([(0, 256 << 21)], 256)
    saved = config.snapshot()
    try:
        for key, value, name in (("output.flac.subtype", "PCM_32", "PCM_32"), ("output.flac.subtype", "FLOAT", "FLOAT"),
                                 ("output.flac.block_size", 4000, "4000"), ("output.flac.md5", "yes", "yes")):
            config.restore(saved)
            config.set_runtime_config({"output.format": "flac", key: value})
            with pytest.raises(ValueError, match=name):
                FX.configured_flac()
            with pytest.raises(ValueError, match=name):
                AE.configured_subtype() if key.endswith("subtype") else AE.configured_flac_options()
        config.restore(saved)
        config.set_runtime_config({"output.format": "flac"})
        assert FX.configured_flac() == {"subtype": "PCM_24", "block_size": 4096, "md5": False}
        assert AE.configured_subtype() == "PCM_24"
        config.set_runtime_config({"output.flac.subtype": "PCM_16", "output.flac.block_size": 512, "output.flac.md5": True})
        assert AE.configured_flac_options() == {"subtype": "PCM_16", "block_size": 512, "md5": True}
        assert AE.configured_subtype() == "PCM_16"
    finally:
        config.restore(saved)


def test_api_refuses_a_bad_flac_key_before_any_work(tmp_path):
    from audio_cut_amd import api
    src = tmp_path / "in.npy"
    np.save(src, np.zeros(100, dtype=np.float32))
    for overrides, name in (({"output.flac.subtype": "PCM_32"}, "PCM_32"), ({"output.flac.block_size": 4000}, "4000")):
        with pytest.raises(ValueError, match=name):
            api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"),
                                     runtime_overrides={"output.format": "flac", **overrides})
    assert not list((tmp_path / "out").glob("*"))


# ---- the export layer on host arrays -------------------------------------------------------------------------------------------
def test_export_audio_and_packed_track_on_the_host(FX, tmp_path):
    rng = np.random.default_rng(5)
    mono = (0.3 * np.sin(np.arange(5000) / 11.0) + 0.01 * rng.standard_normal(5000)).astype(np.float32)
    stereo = np.stack([mono, mono[::-1]])                                              # planar (2, N), as the exporter takes it
    for audio, channels in ((mono, 1), (stereo, 2)):
        for subtype, width in SUBTYPES:
            path = AE.export_audio(audio, SR, tmp_path / f"a_{channels}_{subtype}_1.5", "flac", options={"subtype": subtype, "block_size": 1024})
            assert path.name == f"a_{channels}_{subtype}_1.5.flac"
            wav = AE.export_audio(audio, SR, tmp_path / f"a_{channels}_{subtype}_1.5", "wav", options={"subtype": subtype})
            got, info = flac_decode(path.read_bytes())
            want = FX.pcm_words(wav.read_bytes()[44:], 5000, channels, width)          # the WAV's data chunk
            assert (got == want).all() and info["min_block"] == 1024
    track = AE.PackedTrack(stereo, SR, "PCM_16", flac={"subtype": "PCM_16", "block_size": 256, "md5": True})
    assert track.ext == "flac" and AE.PackedTrack(stereo, SR, "PCM_16").ext == "wav"
    files = AE.SegmentExporter(SR).export_spans(track, [(0, 1000), (1000, 5000)], str(tmp_path / "seg"), segment_is_vocal=[True, False])
    assert [p.rsplit("/", 1)[1] for p in files] == ["segment_001_human.flac", "segment_002_music.flac"]
    pcm, _ = AE.pcm_bytes_host(stereo.T, "PCM_16")
    for path, (lo, hi) in zip(files, ((0, 1000), (1000, 5000))):
        data = open(path, "rb").read()
        got, info = flac_decode(data)
        assert (got == FX.pcm_words(pcm, 5000, 2, 2)[lo:hi]).all()
        assert info["md5"] == hashlib.md5(pcm[4 * lo: 4 * hi].tobytes()).digest()
    with pytest.raises(ValueError, match="PCM_32"):
        AE.export_audio(mono, SR, tmp_path / "b", "flac", options={"subtype": "PCM_32"})
    with pytest.raises(ValueError, match="FLOAT"):
        AE.PackedTrack(mono, SR, "FLOAT", flac={"subtype": "FLOAT", "block_size": 4096})


# ---- nothing changes at the defaults ------------------------------------------------------------------------------------------
def test_defaults_are_untouched():
    assert config.get_config("output.format") == "wav" and config.get_config("output.flac", None) is None
    assert AE.configured_subtype() == "PCM_24" and AE.configured_flac_options() is None
    assert AE.ensure_supported_format(None) == "wav" and AE.ensure_supported_format(" WAV ") == "wav"
    assert AE.ensure_supported_format("FLAC") == "flac"
    with pytest.raises(ValueError, match="mp3"):
        AE.ensure_supported_format("mp3")
    assert AE.build_export_options("wav") == {"subtype": "PCM_24"}
    assert AE.build_export_options("flac") == {"subtype": "PCM_24", "block_size": 4096, "md5": False}
    saved = config.snapshot()
    try:
        for subtype in AE.WAV_SUBTYPES:
            config.set_runtime_config({"output.wav.subtype": subtype})
            assert AE.configured_subtype() == subtype
    finally:
        config.restore(saved)


def test_nothing_of_flac_is_imported_at_the_defaults(tmp_path):
    """A fresh interpreter that exports WAV files from host arrays and reads the configured subtype never imports the FLAC modules."""
    script = (
        "import sys, numpy as np\n"
        "from audio_cut_amd import api\n"
        "from audio_cut_amd.utils import audio_export as AE\n"
        "assert AE.configured_subtype() == 'PCM_24' and AE.configured_flac_options() is None\n"
        f"AE.export_audio(np.zeros(10, dtype=np.float32), 44100, r'{tmp_path}/x', 'wav')\n"
        "t = AE.PackedTrack(np.zeros(10, dtype=np.float32), 44100)\n"
        f"AE.SegmentExporter(44100).export_spans(t, [(0, 5)], r'{tmp_path}', segment_is_vocal=[True])\n"
        "bad = [m for m in sys.modules if m.endswith('flac_export') or m.endswith('_flac_native')]\n"
        "assert not bad, bad\n")
    subprocess.run([sys.executable, "-c", script], check=True, cwd=str(A.ROOT))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
# every export -> the GPU test that calls it directly and compares it with a reference, or "host-only"
FLAC_EXPORTS = ("acl_abi_version", 1, {
    "acl_abi_version": "host-only",
    "acl_last_error": "host-only",
    "acl_flac_plan": "test_flac_export_gpu::test_device_bytes_equal_the_host_statement",
    "acl_flac_write": "test_flac_export_gpu::test_device_bytes_equal_the_host_statement",
})


@pytest.fixture(scope="module")
def flac_lib():
    from audio_cut_amd import _flac_native
    if not _flac_native.library_path().exists():
        subprocess.run(["make", "-C", str(FLAC_CSRC)], check=True)
    return _flac_native.load()


def _prototypes(header):
    """`abi_surface.prototypes` for this library's prefix (that one reads `ac_*` names only): the same reading of the header
    (`A.code`, `A._c_type`), [(return type, name, [parameter types])] of every `acl_*` function; a declaration this cannot read
    is an error."""
    text = re.sub(r"^\s*#[^\n]*", " ", A.code(header), flags=re.M).replace('extern "C" {', " ").replace("}", " ")
    out = []
    for statement in (" ".join(s.split()) for s in text.split(";")):
        if not statement:
            continue
        m = re.fullmatch(r"(.+?)\b(acl_[a-z0-9_]+) ?\(([^()]*)\)", statement)
        assert m, f"{header}: cannot read the declaration {statement!r}"
        params = [] if m.group(3).strip() == "void" else [A._c_type(p, named=True) for p in m.group(3).split(",")]
        out.append((A._c_type(m.group(1), named=False), m.group(2), params))
    return out


def test_flac_surface_against_its_header(flac_lib):
    from audio_cut_amd._flac_native import FLAC_SURFACE as surface, RECORD_INTS
    version_fn, version, export_tests = FLAC_EXPORTS
    assert isinstance(surface, _native.AbiSurface) and surface.header == HEADER
    protos = _prototypes(HEADER)
    names = [name for _, name, _ in protos]
    assert len(set(names)) == len(names) == 4
    assert set(names) == set(surface.signatures) == set(export_tests)
    for name in names:
        assert hasattr(flac_lib, name), f"{name} is declared in {HEADER} but the library does not export it"
    assert version_fn in names and surface.version_fn == version_fn
    assert A.defined_version(HEADER, version_fn) == surface.version == version == getattr(flac_lib, version_fn)()
    for c_res, name, c_params in protos:
        restype, argtypes = surface.signatures[name]
        assert restype is A.ctype(c_res, is_return=True), f"{name}: returns {c_res}, bound as {restype.__name__}"
        want = [A.ctype(p) for p in c_params]
        assert len(argtypes) == len(want), f"{name}: {len(want)} parameters in {HEADER}, {len(argtypes)} argtypes"
        for i, (have, expect) in enumerate(zip(argtypes, want)):
            assert have is expect, f"{name}: parameter {i} is {c_params[i]} in {HEADER}, bound as {have.__name__}"
    (ints,) = re.findall(r"^\s*#define\s+ACL_RECORD_INTS\s+(\d+)", A.code(HEADER), flags=re.M)
    assert int(ints) == RECORD_INTS


def test_flac_surface_is_a_library_of_its_own(flac_lib):
    assert not any(name.startswith("acl_") for name in _native.SIGNATURES)
    assert all(s.header != HEADER for s in _native.ABI_SURFACES)
    assert sorted(p.name for p in (A.INCLUDE / "flac").glob("*.h")) == ["audiocut_flac.h"]
    if _native.library_path().exists():
        main = C.CDLL(str(_native.library_path()))
        for name in FLAC_EXPORTS[2]:
            assert not hasattr(main, name), f"libaudiocut_hip.so exports {name}"
    for name in ("ac_set_error", "ac_last_error", "ac_pack_pcm", "acf_pack_spans", "acf_last_error"):
        assert not hasattr(flac_lib, name), f"libaudiocut_flac.so exports {name}"


def test_flac_makefile_flags_and_the_hook():
    mk = (FLAC_CSRC / "Makefile").read_text()
    (flags,) = re.findall(r"^FLAGS\s*:=(.*)$", mk, flags=re.M)
    (main_flags,) = re.findall(r"^FLAGS\s*:=(.*)$", (A.CSRC / "Makefile").read_text(), flags=re.M)
    assert flags.split() == main_flags.split()
    (nopk,) = re.findall(r"^NOPK\s*:=(.*)$", mk, flags=re.M)
    (main_nopk,) = re.findall(r"^NOPK\s*:=(.*)$", (A.CSRC / "Makefile").read_text(), flags=re.M)
    assert nopk.split() == main_nopk.split() and "-packed-fp32-ops" in nopk
    assert sorted(p.name for p in FLAC_CSRC.glob("*.hip")) == ["ac_flac.hip"] and "ac_flac.hip" in mk
    main = (A.CSRC / "Makefile").read_text()
    assert re.search(r"^all: flac$", main, flags=re.M) and re.search(r"^flac:\n\t\$\(MAKE\) -C flac$", main, flags=re.M)
    (phony,) = re.findall(r"^\.PHONY:(.*)$", main, flags=re.M)
    assert "flac" in phony.split() and re.search(r"^\t\$\(MAKE\) -C flac clean$", main, flags=re.M)


def test_entry_points_refuse_on_the_host(flac_lib):
    """Null pointers, sizes and codes outside the header's ranges: AC_E_INVALID with a text, before anything is launched."""
    lib = flac_lib
    p = 4096        # never dereferenced: the arguments are refused first
    ok_plan = dict(pcm=p, n=100, ch=2, w=3, table=p, rows=1, bs=4096, rec=p, lens=p)
    for change in (dict(pcm=None), dict(table=None), dict(rec=None), dict(lens=None), dict(n=0), dict(n=1 << 40), dict(ch=3),
                   dict(w=4), dict(w=1), dict(rows=0), dict(bs=4000), dict(bs=128), dict(table=p + 4)):
        a = {**ok_plan, **change}
        rc = lib.acl_flac_plan(a["pcm"], a["n"], a["ch"], a["w"], a["table"], a["rows"], a["bs"], a["rec"], a["lens"], None)
        assert rc == -1 and b"invalid argument" in lib.acl_last_error(), change
    ok_write = dict(pcm=p, n=100, ch=1, w=2, table=p, rows=1, bs=256, rate=9, rec=p, offs=p, out=p, total=64)
    for change in (dict(out=None), dict(offs=None), dict(rec=None), dict(rate=12), dict(rate=-1), dict(total=0), dict(bs=100),
                   dict(offs=p + 4)):
        a = {**ok_write, **change}
        rc = lib.acl_flac_write(a["pcm"], a["n"], a["ch"], a["w"], a["table"], a["rows"], a["bs"], a["rate"], a["rec"], a["offs"],
                                a["out"], a["total"], None)
        assert rc == -1 and b"invalid argument" in lib.acl_last_error(), change
