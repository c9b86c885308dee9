"""Segment finishing on the host: `finish_host` against a per-segment restatement written here and against the sample-by-sample
definition, the gain from the sums, the settings and their refusals, the C ABI of libaudiocut_finish.so held against its header,
its binding and the table below (as tests/test_abi_surfaces.py holds the twelve headers of the other library), the host refusals
of both entry points, and that nothing of the feature is imported with the keys at their defaults.  CPU only."""
import ast
import ctypes as C
import math
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_surface as A
from audio_cut_amd import _native, config
from audio_cut_amd.utils import segment_finish as SF

SR = 44100
HEADER = "finish/audiocut_finish.h"
FINISH_CSRC = A.CSRC / "finish"

# every export -> the GPU test that calls it directly and compares it with a reference, or "host-only"
FINISH_EXPORTS = ("acf_abi_version", 1, {
    "acf_abi_version": "host-only",
    "acf_last_error": "host-only",
    "acf_span_stats": "test_segment_finish_gpu::test_span_stats_against_fsum",
    "acf_pack_spans": "test_segment_finish_gpu::test_pack_spans_is_the_host_statement",
})


@pytest.fixture(scope="module")
def finish_lib():
    """libaudiocut_finish.so, built first where it is missing, with every signature declared and its version checked."""
    from audio_cut_amd import _finish_native
    if not _finish_native.library_path().exists():
        subprocess.run(["make", "-C", str(FINISH_CSRC)], check=True)
    return _finish_native.load()


# ---- finish_host ----------------------------------------------------------------------------------------------------------------
def _restated(track, spans, gains, fi, fo):
    """Segment by segment as the reference would: slice, fade the ends in place with np.linspace, multiply by the gain."""
    out = track.copy()
    for (lo, hi), g in zip(spans, gains):
        seg = track[..., lo:hi].copy()
        length = hi - lo
        if fi > 0 and length > fi:
            seg[..., :fi] *= np.linspace(0.0, 1.0, fi)
        if fo > 0 and length > fo:
            seg[..., length - fo:] *= np.linspace(1.0, 0.0, fo)
        seg *= np.float32(g)
        out[..., lo:hi] = seg
    return out


def _by_definition(track, spans, gains, fi, fo):
    """Sample by sample with the closed forms of the weights (include/finish/audiocut_finish.h): what the kernels compute."""
    out = track.copy()
    flat = out.reshape(-1, out.shape[-1])
    for (lo, hi), g in zip(spans, gains):
        length = hi - lo
        for row in flat:
            for f in range(lo, hi):
                i, v = f - lo, row[f]
                if fi > 0 and length > fi and i < fi:
                    w = (0.0 if fi == 1 else 1.0) if i == fi - 1 else i * (1.0 / (fi - 1))
                    v = np.float32(np.float64(v) * w)
                if fo > 0 and length > fo and i >= length - fo:
                    j = i - (length - fo)
                    w = (1.0 if fo == 1 else 0.0) if j == fo - 1 else np.float64(j * (-1.0 / (fo - 1))) + 1.0
                    v = np.float32(np.float64(v) * w)
                row[f] = np.float32(v) * np.float32(g)
    return out


def _layout(lengths, gaps):
    spans, pos = [], 0
    for k, length in enumerate(lengths):
        pos += gaps[k % len(gaps)]
        spans.append((pos, pos + length))
        pos += length
    return spans, pos + 1 + gaps[len(lengths) % len(gaps)]


@pytest.mark.parametrize("channels", [1, 2])
def test_finish_host_is_the_per_segment_restatement(channels):
    rng = np.random.default_rng(channels)
    for fi in (0, 1, 2, 441):
        for fo in (0, 1, 2, 441):
            lengths = sorted({v for v in (1, fi, fi + 1, fi + fo - 1, fi + fo, 5000) if v > 0})
            spans, n = _layout(lengths, gaps=(3, 2, 0, 1, 7))
            assert any(b < c for (_, b), (c, _) in zip(spans, spans[1:])) and spans[0][0] > 0 and spans[-1][1] < n      # gaps
            track = (0.6 * rng.standard_normal((channels, n) if channels == 2 else n)).astype(np.float32)
            gains = rng.choice(np.array([1.0, 0.37, 3.0, 10.0], dtype=np.float32), len(spans))
            got = SF.finish_host(track, spans, gains, fi, fo)
            assert got.dtype == np.float32 and got.shape == track.shape
            assert got.tobytes() == _restated(track, spans, gains, fi, fo).tobytes(), (fi, fo)
            outside = np.ones(n, dtype=bool)
            for lo, hi in spans:
                outside[lo:hi] = False
            assert got[..., outside].tobytes() == track[..., outside].tobytes()


@pytest.mark.parametrize("channels", [1, 2])
def test_finish_host_is_the_sample_by_sample_definition(channels):
    rng = np.random.default_rng(10 + channels)
    for fi, fo in ((0, 0), (1, 1), (2, 0), (0, 2), (7, 3), (3, 7), (7, 7)):
        lengths = sorted({v for v in (1, 2, fi, fi + 1, fi + fo - 1, fi + fo, fi + fo + 1, 40) if v > 0})
        spans, n = _layout(lengths, gaps=(2, 0, 1))
        track = (0.6 * rng.standard_normal((channels, n) if channels == 2 else n)).astype(np.float32)
        gains = rng.choice(np.array([1.0, 0.37, 3.0], dtype=np.float32), len(spans))
        assert SF.finish_host(track, spans, gains, fi, fo).tobytes() == _by_definition(track, spans, gains, fi, fo).tobytes(), (fi, fo)


def test_the_closed_forms_are_linspace():
    for f in (1, 2, 3, 7, 441, 882, 44100):
        up = np.array([(0.0 if f == 1 else 1.0) if i == f - 1 else i * (1.0 / (f - 1)) for i in range(f)])
        down = np.array([(1.0 if f == 1 else 0.0) if j == f - 1 else np.float64(j * (-1.0 / (f - 1))) + 1.0 for j in range(f)])
        assert up.tobytes() == np.linspace(0, 1, f).tobytes() and down.tobytes() == np.linspace(1, 0, f).tobytes(), f


def test_finish_host_refuses_bad_spans():
    x = np.zeros(100, dtype=np.float32)
    for spans in ([(10, 5)], [(5, 5)], [(0, 101)], [(-1, 5)], [(20, 30), (10, 15)], [(0, 10), (9, 12)]):
        with pytest.raises(ValueError, match="spans"):
            SF.finish_host(x, spans, np.ones(len(spans), np.float32), 2, 2)
    with pytest.raises(ValueError, match="gain"):
        SF.finish_host(x, [(0, 10)], np.ones(2, np.float32), 0, 0)


def test_finish_stats_host_and_the_host_track():
    """`PackedTrack.finished` without a context: `finish_host` through `pcm_bytes_host`, the rows from `finish_stats_host`."""
    from audio_cut_amd.utils import audio_export as AE
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal((2, 3000))).astype(np.float32)
    x[:, 2000:2500] = 0.0
    spans = [(7, 1200), (1200, 1999), (2000, 2500)]
    st = SF.finish_settings({"fade_in_duration": 0.001, "fade_out_duration": 0.002, "normalize_audio": True}, SR)
    assert (st.fade_in_frames, st.fade_out_frames) == (44, 88)
    sumsq, peak = SF.finish_stats_host(x, spans, 44, 88)
    faded = SF.finish_host(x, spans, np.ones(3, np.float32), 44, 88)
    for k, (lo, hi) in enumerate(spans):
        seg = faded[:, lo:hi].astype(np.float64)
        assert sumsq[k] == math.fsum((seg * seg).reshape(-1).tolist()) and peak[k] == np.abs(faded[:, lo:hi]).max()
    gains = np.array([SF.gain_from_stats(s, (hi - lo) * 2, st) for s, (lo, hi) in zip(sumsq, spans)], dtype=np.float32)
    assert gains[2] == 1.0 and gains[0] != 1.0
    track = AE.PackedTrack.finished(x, SR, spans, st, "PCM_16")
    want, _ = AE.pcm_bytes_host(SF.finish_host(x, spans, gains, 44, 88).T, "PCM_16")
    assert (track.n, track.channels, track.width, track.subtype) == (3000, 2, 2, "PCM_16")
    assert np.asarray(track.bytes).tobytes() == want.tobytes()
    rows = track.finish_rows
    assert [set(r) for r in rows] == [{"gain", "gain_db", "rms_db", "peak_out", "clipped"}] * 3
    assert [r["gain"] for r in rows] == [float(g) for g in gains]
    assert rows[0]["rms_db"] == pytest.approx(10.0 * math.log10(sumsq[0] / (1193 * 2))) and rows[2]["rms_db"] is None
    assert rows[0]["peak_out"] == float(np.float32(peak[0]) * gains[0]) and rows[0]["clipped"] == (rows[0]["peak_out"] >= 1.0)
    loud = AE.PackedTrack.finished(np.full(100, 0.5, np.float32), SR, [(0, 100)],
                                   SF.finish_settings({"normalize_audio": True, "normalize_target_db": 6.0}, SR), "PCM_16")
    assert loud.finish_rows[0]["clipped"] is True and loud.finish_rows[0]["gain"] == float(np.float32(10 ** 0.3 / 0.5))
    quiet = AE.PackedTrack.finished(np.full(100, 0.5, np.float32), SR, [(0, 100)],
                                    SF.finish_settings({"normalize_audio": True, "normalize_target_db": 6.0}, SR), "FLOAT")
    assert quiet.finish_rows[0]["clipped"] is False                     # the float subtypes do not clip
    # only fades: nothing is measured, the gains are 1
    plain = AE.PackedTrack.finished(x, SR, spans, SF.finish_settings({"fade_in_duration": 0.001}, SR), "FLOAT")
    assert [r["gain"] for r in plain.finish_rows] == [1.0] * 3 and plain.finish_rows[0]["rms_db"] is None
    assert np.asarray(plain.bytes).tobytes() == AE.pcm_bytes_host(SF.finish_host(x, spans, np.ones(3, np.float32), 44, 0).T, "FLOAT")[0].tobytes()


# ---- gain_from_stats ------------------------------------------------------------------------------------------------------------
def test_gain_from_stats():
    on = SF.finish_settings({"normalize_audio": True}, SR)
    assert SF.gain_from_stats(0.0, 1000, on) == np.float32(1.0)                                    # silence
    assert SF.gain_from_stats(float("nan"), 1000, on) == np.float32(1.0)
    assert SF.gain_from_stats(float("inf"), 1000, on) == np.float32(1.0)
    # a full-scale sine over whole periods: sumsq = n / 2, rms = sqrt(1 / 2), g = 10^(-20 / 20) / sqrt(1 / 2) = 0.1 * sqrt(2)
    n = 44100
    g = SF.gain_from_stats(n / 2.0, n, on)
    assert isinstance(g, np.float32) and g == np.float32(0.1 * math.sqrt(2.0))
    x = np.sin(2 * np.pi * 100.0 * np.arange(n) / n).astype(np.float32)
    sumsq, _ = SF.finish_stats_host(x, [(0, n)], 0, 0)
    assert abs(float(SF.gain_from_stats(sumsq[0], n, on)) - 0.1 * math.sqrt(2.0)) < 1e-6
    assert SF.gain_from_stats(1e-12 * n, n, on) == np.float32(10.0)                               # rms 1e-6: the cap
    capped = SF.finish_settings({"normalize_audio": True, "normalize_max_gain": 2.5, "normalize_target_db": -6.0}, SR)
    assert SF.gain_from_stats(1e-6 * n, n, capped) == np.float32(2.5)
    assert SF.gain_from_stats(1.0 * n, n, capped) == np.float32(10.0 ** (-6.0 / 20.0))
    off = SF.finish_settings({"fade_in_duration": 0.01}, SR)
    assert SF.gain_from_stats(n / 2.0, n, off) == np.float32(1.0)


# ---- configured_finish ----------------------------------------------------------------------------------------------------------
def _configured(overrides, sr=SR):
    saved = config.snapshot()
    try:
        config.set_runtime_config({f"quality_control.{k}": v for k, v in overrides.items()}, explicit=False)
        return SF.configured_finish(sr)
    finally:
        config.restore(saved)


def test_configured_finish():
    for key, default in (("fade_in_duration", 0.0), ("fade_out_duration", 0.0), ("normalize_audio", False),
                         ("normalize_target_db", -20.0), ("normalize_max_gain", 10.0)):
        value = config.get_config(f"quality_control.{key}", "missing")
        assert value == default and type(value) is type(default), key
    st = _configured({})
    assert st.active is False and (st.fade_in_frames, st.fade_out_frames, st.normalize_audio) == (0, 0, False)
    assert (st.normalize_target_db, st.normalize_max_gain) == (-20.0, 10.0)
    assert _configured({"normalize_target_db": -14.0, "normalize_max_gain": 4.0}).active is False   # they switch nothing on
    st = _configured({"fade_in_duration": 0.01, "fade_out_duration": 0.0101})
    assert st.active and (st.fade_in_frames, st.fade_out_frames) == (441, 445) and not st.normalize_audio    # int(d * sr) truncates
    assert _configured({"fade_out_duration": 0.02}, sr=48000).fade_out_frames == 960
    assert _configured({"fade_in_duration": 1e-6}).active is False                                 # less than a frame
    st = _configured({"normalize_audio": True, "normalize_target_db": -14, "normalize_max_gain": 4})
    assert st.active and st.normalize_audio and (st.normalize_target_db, st.normalize_max_gain) == (-14.0, 4.0)
    refused = {"fade_in_duration": (-0.01, float("nan"), float("inf"), "10ms"), "fade_out_duration": (-1, float("-inf"), [0.01]),
               "normalize_target_db": (float("nan"), float("inf"), "loud"), "normalize_max_gain": (0, -1.0, float("nan")),
               "normalize_audio": ("yes", 1)}
    for key, values in refused.items():
        for value in values:
            with pytest.raises(ValueError, match=rf"quality_control\.{key}\b"):
                _configured({key: value})


# ---- the ABI of libaudiocut_finish.so ----------------------------------------------------------------------------------------------
def _prototypes(header):
    """`abi_surface.prototypes` for this library's prefix (that one reads `ac_*` names only): the same reading of the header
    (`A.code`, `A._c_type`), [(return type, name, [parameter types])] of every `acf_*` function; a declaration this cannot read is
    an error."""
    text = re.sub(r"^\s*#[^\n]*", " ", A.code(header), flags=re.M).replace('extern "C" {', " ").replace("}", " ")
    out = []
    for statement in (" ".join(s.split()) for s in text.split(";")):
        if not statement:
            continue
        m = re.fullmatch(r"(.+?)\b(acf_[a-z0-9_]+) ?\(([^()]*)\)", statement)
        assert m, f"{header}: cannot read the declaration {statement!r}"
        params = [] if m.group(3).strip() == "void" else [A._c_type(p, named=True) for p in m.group(3).split(",")]
        out.append((A._c_type(m.group(1), named=False), m.group(2), params))
    return out


def test_finish_header_registry_library_and_table_are_one_surface(finish_lib):
    from audio_cut_amd._finish_native import FINISH_SURFACE as surface
    version_fn, version, export_tests = FINISH_EXPORTS
    assert isinstance(surface, _native.AbiSurface) and surface.header == HEADER
    protos = _prototypes(HEADER)
    names = [name for _, name, _ in protos]
    assert len(set(names)) == len(names) == 4
    assert set(names) == set(surface.signatures) == set(export_tests)
    for name in names:
        assert hasattr(finish_lib, name), f"{name} is declared in {HEADER} but the library does not export it"
    assert version_fn in names and surface.version_fn == version_fn
    assert A.defined_version(HEADER, version_fn) == surface.version == version == getattr(finish_lib, version_fn)()
    for c_res, name, c_params in protos:
        restype, argtypes = surface.signatures[name]
        assert restype is A.ctype(c_res, is_return=True), f"{name}: returns {c_res}, bound as {restype.__name__}"
        want = [A.ctype(p) for p in c_params]
        assert len(argtypes) == len(want), f"{name}: {len(want)} parameters in {HEADER}, {len(argtypes)} argtypes"
        for i, (got, exp) in enumerate(zip(argtypes, want)):
            assert got is exp, f"{name}: parameter {i} is {c_params[i]} in {HEADER}, bound as {got.__name__}"
        assert getattr(finish_lib, name).restype is restype and list(getattr(finish_lib, name).argtypes) == list(argtypes)
    for name, ref in export_tests.items():
        if ref != "host-only":
            module, test = ref.split("::")
            tree = ast.parse((A.ROOT / "tests" / f"{module}.py").read_text())
            assert test in {node.name for node in tree.body if isinstance(node, ast.FunctionDef)}, f"{name}: {ref} does not exist"
            assert module.endswith("_gpu"), f"{name}: {ref} is not a GPU test"


def test_the_two_libraries_keep_their_names_apart(finish_lib):
    """Nothing of this library is declared or bound in the other one's registry, and the other library exports no `acf_*` name."""
    assert not any(name.startswith("acf_") for name in _native.SIGNATURES)
    assert sorted(p.name for p in (A.INCLUDE / "finish").glob("*.h")) == ["audiocut_finish.h"]
    if _native.library_path().exists():
        main = C.CDLL(str(_native.library_path()))
        for name in FINISH_EXPORTS[2]:
            assert not hasattr(main, name), f"libaudiocut_hip.so exports {name}"
    for name in ("ac_set_error", "ac_last_error", "ac_pack_pcm"):
        assert not hasattr(finish_lib, name), f"libaudiocut_finish.so exports {name}"


def test_finish_makefile_flags_and_the_first_target():
    mk = (FINISH_CSRC / "Makefile").read_text()
    (flags,) = re.findall(r"^FLAGS\s*:=(.*)$", mk, flags=re.M)
    assert "-ffp-contract=off" in flags.split() and "$(NOPK)" in flags.split() and "--offload-arch=$(ARCH)" in flags.split()
    (nopk,) = re.findall(r"^NOPK\s*:=(.*)$", mk, flags=re.M)
    (main_nopk,) = re.findall(r"^NOPK\s*:=(.*)$", (A.CSRC / "Makefile").read_text(), flags=re.M)
    assert nopk.split() == main_nopk.split() and "-packed-fp32-ops" in nopk
    assert sorted(p.name for p in FINISH_CSRC.glob("*.hip")) == ["ac_finish.hip"] and "ac_finish.hip" in mk
    main = (A.CSRC / "Makefile").read_text()
    first = re.search(r"^([A-Za-z_$()][^:=\n]*):(?!=)(.*)$", main, flags=re.M)
    assert first and first.group(1).strip() == "all" and first.group(2).split() == ["$(OUT)", "finish"]
    assert re.search(r"^finish:\n\t\$\(MAKE\) -C finish$", main, flags=re.M)


# ---- host refusals of the entry points ----------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host(finish_lib):
    lib = finish_lib
    real = C.create_string_buffer(64)
    p = (C.addressof(real) + 15) & ~15                                        # 16-byte aligned, never dereferenced: every call below is refused

    def err():
        return lib.acf_last_error().decode()

    def pack(x=p, n=8, ch=1, stride=8, a=p, b=p, g=p, k=1, fi=0, fo=0, st=4, out=p):
        return lib.acf_pack_spans(x, n, ch, stride, a, b, g, k, fi, fo, st, out, None)

    def stats(x=p, n=8, ch=1, stride=8, a=p, b=p, k=1, fi=0, fo=0, ss=p, pk=p):
        return lib.acf_span_stats(x, n, ch, stride, a, b, k, fi, fo, ss, pk, None)

    for call, what in ((lambda: pack(x=None), "null"), (lambda: pack(a=None), "null"), (lambda: pack(b=None), "null"),
                       (lambda: pack(g=None), "null"), (lambda: pack(out=None), "null"), (lambda: pack(n=0), "n_frames"),
                       (lambda: pack(n=-3), "n_frames"), (lambda: pack(n=1 << 40), "too long"), (lambda: pack(ch=0), "channels"),
                       (lambda: pack(ch=3), "channels"), (lambda: pack(ch=2, stride=7), "row_stride"), (lambda: pack(k=0), "n_spans"),
                       (lambda: pack(k=-1), "n_spans"), (lambda: pack(fi=-1), "fades"), (lambda: pack(fo=-1), "fades"),
                       (lambda: pack(st=6), "subtype"), (lambda: pack(st=-1), "subtype"), (lambda: pack(x=p + 2), "aligned"),
                       (lambda: pack(out=p + 4, st=4), "aligned"), (lambda: pack(out=p + 4, st=1), "aligned"),
                       (lambda: pack(out=p + 2, st=0), "aligned"),
                       (lambda: stats(x=None), "null"), (lambda: stats(a=None), "null"), (lambda: stats(b=None), "null"),
                       (lambda: stats(ss=None), "null"), (lambda: stats(pk=None), "null"), (lambda: stats(n=0), "n_frames"),
                       (lambda: stats(n=1 << 40), "too long"), (lambda: stats(ch=3), "channels"),
                       (lambda: stats(ch=2, stride=7), "row_stride"), (lambda: stats(k=0), "n_spans"), (lambda: stats(fi=-1), "fades"),
                       (lambda: stats(fo=-2), "fades"), (lambda: stats(x=p + 1), "aligned")):
        assert call() == -1 and err().startswith("invalid argument") and what in err(), (what, err())


# ---- off is off -------------------------------------------------------------------------------------------------------------------
_OFF_IS_OFF = r"""
import sys
sys.path.insert(0, {root!r})
from pathlib import Path
from audio_cut_amd import api, config

class Stop(Exception):
    pass

def stop(*a, **k):          # the first thing `_split_and_export` does after reading its settings: nothing touches a GPU
    raise Stop

api.SeamlessSplitter = stop
NEW = ("audio_cut_amd.utils.segment_finish", "audio_cut_amd._finish_native")

def run(overrides):
    saved = config.snapshot()
    config.set_runtime_config(overrides, explicit=False)
    try:
        api._split_and_export(Path("song.npy"), Path("."), "v2.2_mdd", None, 44100, None)
    except Stop:
        return [m in sys.modules for m in NEW]
    finally:
        config.restore(saved)

assert run({{}}) == [False, False], "the defaults import the feature"
assert run({{"quality_control.normalize_target_db": -20.0, "quality_control.fade_in_duration": 0}}) == [False, False]
assert run({{"quality_control.fade_in_duration": 0.01}}) == [True, False], "the library is opened only when a track is finished"
try:
    run({{"quality_control.fade_out_duration": -1.0}})
except ValueError as e:
    assert "quality_control.fade_out_duration" in str(e)
else:
    raise AssertionError("a negative fade was not refused before any work")
print("off is off")
"""


def test_off_is_off():
    """With the keys at their defaults `_split_and_export` imports nothing of the feature; with one set, the settings are read (and
    refused) before any work.  A fresh process that stops in front of any GPU use."""
    done = subprocess.run([sys.executable, "-c", _OFF_IS_OFF.format(root=str(A.ROOT))], capture_output=True, text=True, cwd=str(A.ROOT))
    assert done.returncode == 0 and done.stdout.strip().endswith("off is off"), done.stdout + done.stderr
