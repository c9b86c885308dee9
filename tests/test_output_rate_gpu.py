"""`output.sample_rate` on the device (GPU box only): `ac_resample_poly_pack` (include/audiocut_hip_rate.h) against the composition
it replaces - `ac_resample_poly` per channel, then `ac_pack_pcm` - byte for byte, against its host statement
(`utils/rate_export.py: resample_pack_host`), under poisoned and guarded allocations, at its refusals, and through
`separate_and_segment` on a 48 kHz stereo file.

Comparisons with the device composition are exact.  Comparisons with the host statement are exact wherever the float the device
resampler gives is the host's (the float64 sum rounded once); elsewhere the device float is a neighbour of it (the device adds 64
float64 partial sums in another order), and the word may differ by one step.  The share of such floats is capped at 1e-3, so that
a wrong tap - which moves every output - cannot hide behind the allowance.  Observed on the MI355X with SEED below: see
OBSERVED_SHARE."""
import functools
import json
import wave

import numpy as np
import pytest
import torch

import resample_refs as R
from audio_cut_amd import api
from audio_cut_amd._native import Context, NativeError, _check, _stream
from audio_cut_amd.testing import signals
from audio_cut_amd.utils import audio_export as AE
from audio_cut_amd.utils import rate_export as RE
from poison_alloc import run_three

pytestmark = pytest.mark.gpu
SR = 44100
RATIOS = [(160, 147), (147, 160), (320, 147), (2, 1), (1, 2), (80, 441)]
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 1023, 4097]      # shorter than the filter's half length .. many workgroups; groups of 8 words cut everywhere
SUBTYPES = list(AE.WAV_SUBTYPES)
SEED = 20261
PAD = 5                                              # the stereo rows are views into rows this much longer: row_stride > n
SHARE_CAP = 1e-3
# Share of ac_resample_poly's floats that differ from float32(polyphase_ref64) with SEED, n = 4097, mono, measured once on the
# MI355X (test_the_seed_keeps_the_shipped_resampler_under_the_cap prints it): 0 of 28 131 outputs over the six ratios; and 0 of
# 110 986 against the host statement over every track of test_kernel_is_the_composition_and_the_host_statement.
OBSERVED_SHARE = 0.0


@functools.lru_cache(maxsize=None)
def track(n):
    """[3, n + PAD] float32, read-only: row 0 is the mono track, rows 1 and 2 the stereo pair (their first n samples).  Gaussian
    noise x 1.5, so both clipping branches of the integer conversions occur, with exact +-1.0, +-0.0 and +-denormals planted,
    evenly spread: at most one sample in four is a planted one (n = 7: +1.0 alone; n = 1: none), so every output has noise among
    its terms.  A track of planted values ALONE has outputs where +1.0 and -1.0 meet equal taps of the symmetric filter and cancel
    exactly, leaving a sum of 1e-42: there the device's float64 sum, taken over 64 lanes in another order than the host's, loses
    the small terms behind the large ones (0.0 against -1.4e-42, seen at 2/1, n = 7) - inside ac_resample_poly's own bound
    (tpp 2^-52 of the sum of |terms|, tests/resample_refs.py), but no neighbour of the host's float, which is what this file
    holds the words outside the exact set to."""
    x = (np.random.default_rng(SEED + n).standard_normal((3, n + PAD)) * 1.5).astype(np.float32)
    plant = np.float32([1.0, -1.0, 0.0, -0.0, 1e-41, -1e-41, 2.0 ** -149])[: n // 4]
    for r in range(3):
        if plant.size:
            x[r, (np.arange(plant.size) * (n // plant.size) + r) % n] = plant
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def host_floats(up, down, n):
    """[3, ceil(n up / down)] float32: the host statement of every row of track(n), computed once and shared (read-only)."""
    x = track(n)[:, :n]
    y = np.stack([RE.resample_host(row, up, down, R.n_out_of(n, up, down)) for row in x])
    y.setflags(write=False)
    return y


def words(data: np.ndarray, subtype: str) -> np.ndarray:
    """Sample bytes -> one int64 (integer subtypes) or float64 (FLOAT, DOUBLE) per word."""
    data = np.ascontiguousarray(data)
    if subtype == "PCM_U8":
        return data.astype(np.int64)
    if subtype == "PCM_16":
        return data.view("<i2").astype(np.int64)
    if subtype == "PCM_24":
        b = data.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return np.where(v & 0x800000, v - 0x1000000, v)
    if subtype == "PCM_32":
        return data.view("<i4").astype(np.int64)
    return data.view("<f4" if subtype == "FLOAT" else "<f8").astype(np.float64)


def assert_one_step(got: np.ndarray, want: np.ndarray, subtype: str, label: str) -> None:
    """Words converted from neighbouring float32 values: at most 1 LSB apart (integer subtypes), at most one float32 ulp (FLOAT,
    and DOUBLE, whose words are float32 values widened exactly)."""
    if got.size == 0:
        return
    if subtype in ("FLOAT", "DOUBLE"):
        assert np.all(np.abs(got - want) <= R.ulp32(np.maximum(np.abs(got), np.abs(want)))), label
    else:
        assert int(np.max(np.abs(got - want))) <= 1, (label, int(np.max(np.abs(got - want))))


@pytest.mark.parametrize("up,down", RATIOS)
def test_kernel_is_the_composition_and_the_host_statement(hip_ctx, up, down):
    differ = total = launches = 0
    for n in LENGTHS:
        x = track(n)
        dev = hip_ctx.to_device(x.copy())
        n_full = R.n_out_of(n, up, down)
        floats = torch.stack([hip_ctx.resample_poly(dev[r, :n].contiguous(), up, down) for r in range(3)])       # [3, n_full]
        assert floats.shape == (3, n_full)
        href = host_floats(up, down, n)
        same = floats.cpu().numpy() == href                                                        # [3, n_full]
        differ, total = differ + int(np.count_nonzero(~same)), total + same.size
        for layout in ("mono", "stereo"):
            src = dev[0, :n] if layout == "mono" else dev[1:3, :n]                                 # stereo: row_stride n + PAD
            comp_src = floats[0] if layout == "mono" else floats[1:3]
            if layout == "stereo":
                assert src.stride(0) == n + PAD > n and not src.is_contiguous()
            for crop in (0, 1, 2):
                n_out = n_full - crop
                if n_out < 1:
                    continue
                mask = same[0, :n_out] if layout == "mono" else same[1:3, :n_out].T.reshape(-1)     # per word, frames interleaved
                for subtype in SUBTYPES:
                    label = f"{up}/{down} n={n} {layout} crop={crop} {subtype}"
                    got = RE.resample_pack_device(hip_ctx, src, up, down, subtype, n_out if (crop or layout == "stereo") else None)
                    launches += 1
                    want = hip_ctx.pack_pcm_device(comp_src[..., :n_out], subtype)
                    assert got.dtype == torch.uint8 and got.shape == want.shape == (n_out * (1 if layout == "mono" else 2) * AE.WAV_SUBTYPES[subtype][1],)
                    assert torch.equal(got, want), label
                    # the host statement: pcm_bytes_host of the shared host floats, which is resample_pack_host (asserted once
                    # per track and layout, for the rest tests/test_output_rate_host.py holds the two together)
                    hf = href[0, :n_out] if layout == "mono" else href[1:3, :n_out].T
                    h = AE.pcm_bytes_host(hf, subtype)[0]
                    if crop == 1 and subtype == "PCM_24":
                        assert np.array_equal(h, RE.resample_pack_host(x[0, :n] if layout == "mono" else x[1:3, :n], up, down, subtype, n_out))
                    width = AE.WAV_SUBTYPES[subtype][1]
                    g = got.cpu().numpy()
                    assert g.shape == h.shape
                    assert np.array_equal(g.reshape(-1, width)[mask], h.reshape(-1, width)[mask]), label
                    assert_one_step(words(g, subtype)[~mask], words(h, subtype)[~mask], subtype, label)
    share = differ / total
    print(f"resample_pack {up}/{down}: {launches} launches equal the composition byte for byte; {differ} of {total} device floats "
          f"differ from the host statement (share {share:.2e}, cap {SHARE_CAP:g})")
    assert share < SHARE_CAP


def test_the_seed_keeps_the_shipped_resampler_under_the_cap(hip_ctx):
    """`ac_resample_poly` itself against float32(polyphase_ref64) - the correctly rounded sum - on the mono track of n = 4097."""
    differ = total = 0
    for up, down in RATIOS:
        hfull, npr = Context._resample_filter(up, down)
        x = track(4097)[0, :4097]
        y64, _ = R.polyphase_ref64(x, up, down, hfull, npr, R.n_out_of(4097, up, down))
        got = hip_ctx.resample_poly(hip_ctx.to_device(x.copy()), up, down).cpu().numpy()
        differ, total = differ + int(np.count_nonzero(got != y64.astype(np.float32))), total + got.size
    print(f"ac_resample_poly vs float32(polyphase_ref64), SEED {SEED}: {differ} of {total} differ (share {differ / total:.2e})")
    assert differ / total < SHARE_CAP


@pytest.mark.parametrize("layout,subtype", [("stereo", "PCM_24"), ("mono", "DOUBLE")])
def test_poisoned_and_guarded(hip_ctx, layout, subtype):
    """Every byte of the result is written (two poisons, one result), nothing around `out` is touched, and reads outside the
    input do not reach the result."""
    n, (up, down) = 4097, (160, 147)
    x = track(n)[1:3, :n] if layout == "stereo" else track(n)[0, :n]
    n_out = R.n_out_of(n, up, down) - 1
    hip_ctx._resample_filter_dev(up, down)                              # designed and uploaded outside the poisoned runs
    x = np.array(x)                                                    # a contiguous, writable copy
    got = run_three(hip_ctx, lambda upload: RE.resample_pack_device(hip_ctx, upload(x), up, down, subtype, n_out))
    d = hip_ctx.to_device(x)
    floats = torch.stack([hip_ctx.resample_poly(d[c].contiguous(), up, down) for c in range(2)]) if layout == "stereo" \
        else hip_ctx.resample_poly(d, up, down)
    assert torch.equal(got, hip_ctx.pack_pcm_device(floats[..., :n_out], subtype))
    assert got.numel() == n_out * (2 if layout == "stereo" else 1) * AE.WAV_SUBTYPES[subtype][1]


def test_refusals_launch_nothing(hip_ctx):
    n, (up, down) = 65, (160, 147)
    n_full = R.n_out_of(n, up, down)
    x = hip_ctx.to_device(track(n)[:, :n].copy())                       # [3, n] contiguous
    with pytest.raises(NativeError, match="n_out"):
        RE.resample_pack_device(hip_ctx, x[0], up, down, "PCM_16", n_full + 1)
    with pytest.raises(NativeError):
        RE.resample_pack_device(hip_ctx, x[0], up, down, "PCM_16", 0)
    with pytest.raises(NativeError, match=r"\[n\] or \[2, n\]"):
        RE.resample_pack_device(hip_ctx, x, up, down, "PCM_16")         # three rows
    with pytest.raises(ValueError, match="ULAW"):
        RE.resample_pack_device(hip_ctx, x[0], up, down, "ULAW")
    # the entry point itself: channels 3, an unknown subtype code, a misaligned `out`, n_out too large
    hd, npr = hip_ctx._resample_filter_dev(up, down)
    out = torch.full((n_full * 2 * 8 + 64,), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    assert out.data_ptr() % 16 == 0
    call = hip_ctx.lib.ac_resample_poly_pack

    def args(channels=2, subtype=1, out_ptr=out.data_ptr(), n_out=n_full):
        return (hip_ctx._h, x.data_ptr(), n, channels, n, up, down, hd.data_ptr(), hd.numel(), npr, subtype, out_ptr, n_out, _stream())

    for kw, word in (({"channels": 3}, "channels"), ({"subtype": 6}, "subtype"), ({"subtype": 1, "out_ptr": out.data_ptr() + 4}, "aligned"),
                     ({"subtype": 5, "out_ptr": out.data_ptr() + 8}, "aligned"), ({"subtype": 2, "out_ptr": out.data_ptr() + 2}, "aligned"),
                     ({"n_out": n_full + 1}, "n_out")):
        with pytest.raises(NativeError, match=word):
            _check(call(*args(**kw)))
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                    # nothing was launched
    _check(call(*args()))                                               # and the same arguments, unrefused, write
    torch.cuda.synchronize()
    assert torch.equal(out[: n_full * 2 * 2], RE.resample_pack_device(hip_ctx, x[0:2], up, down, "PCM_16")) and bool((out[n_full * 4:] == 0xA5).all())


def test_equal_rates_are_pack_pcm(hip_ctx):
    x = hip_ctx.to_device(track(1023)[1:3, :1023].copy())
    for subtype in ("PCM_24", "FLOAT"):
        assert torch.equal(RE.resample_pack_device(hip_ctx, x, 48000, 48000, subtype), hip_ctx.pack_pcm_device(x, subtype))
        assert torch.equal(RE.resample_pack_device(hip_ctx, x[0], 3, 3, subtype, 1000), hip_ctx.pack_pcm_device(x[0, :1000], subtype))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _wav(path):
    with wave.open(str(path), "rb") as w:
        return w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.readframes(w.getnframes())


@pytest.fixture(scope="module")
def runs(hip_ctx, tmp_path_factory):
    """The 48 kHz stereo 16-bit file of test_separate_and_segment_with_two_channels, exported at its own rate and, a second time,
    without the setting; and the same track straight through split_track.  Computed once, read by the tests below."""
    import scipy.signal
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    root = tmp_path_factory.mktemp("rate")
    st = signals.c2_song(14.0, seed=9, stereo=True)
    st48 = np.stack([scipy.signal.resample_poly(ch, 160, 147) for ch in st]).astype(np.float32)
    src = root / "song48.wav"
    pcm = np.clip(np.rint(st48.T * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(src), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(pcm.tobytes())
    base = {"audio.channels": 2, "output.wav.subtype": "PCM_16"}
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(root / "source"), export_manifest=True,
                                   runtime_overrides={**base, "output.sample_rate": "source"})
    res = api.last_result()
    plain_man = api.separate_and_segment(input_uri=str(src), export_dir=str(root / "plain"), export_manifest=True, runtime_overrides=base)
    plain = api.last_result()
    loaded, file_sr = api.load_audio_stereo(str(src))
    st44_dev = torch.stack([hip_ctx.resample_poly(hip_ctx.to_device(loaded[c]), SR, file_sr) for c in range(2)])
    direct = SeamlessSplitter(SR).split_track(st44_dev.cpu().numpy())
    return {"src": src, "pcm": pcm, "man": man, "res": res, "plain_man": plain_man, "plain": plain, "direct": direct,
            "st44": st44_dev.cpu().numpy(), "root": root}


def _direct_spans(direct):
    cuts = direct["cuts_samples"]
    return [tuple(sp) for sp in direct.get("segment_spans", list(zip(cuts[:-1], cuts[1:])))]


def test_source_rate_every_file_is_at_the_files_rate_and_the_mix_is_the_file(runs):
    res, pcm = runs["res"], runs["pcm"]
    n_src = pcm.shape[0]
    assert res["num_segments"] >= 2 and len(res["mix_segment_files"]) == len(res["vocal_segment_files"]) == res["num_segments"]
    assert res["full_vocal_file"] and res["full_instrumental_file"] and len(res["saved_files"]) == 2 * res["num_segments"] + 2
    for f in res["saved_files"]:
        ch, width, rate, _, _ = _wav(f)
        assert (ch, width, rate) == (2, 2, 48000), f
    # the mix segments, concatenated, are the source's data chunk byte for byte: nothing was resampled twice
    assert b"".join(_wav(f)[4] for f in res["mix_segment_files"]) == pcm.tobytes()
    for f in (res["full_vocal_file"], res["full_instrumental_file"]):
        assert _wav(f)[3] == n_src


def test_source_rate_stems_are_the_kernel_on_the_resident_stems(hip_ctx, runs):
    res, direct, n_src = runs["res"], runs["direct"], runs["pcm"].shape[0]
    n = runs["st44"].shape[1]
    assert n == -(-n_src * 147 // 160) and n_src <= RE.resampled_len(n, 160, 147) <= n_src + 2
    voc_dev = direct["device_state"]["vocal_stereo"]
    assert np.array_equal(voc_dev.cpu().numpy(), direct["vocal_track_stereo"])
    # the device composition of the direct run's stem, cropped to the file's frames
    floats = torch.stack([hip_ctx.resample_poly(voc_dev[c].contiguous(), 160, 147) for c in range(2)])[:, :n_src]
    want = hip_ctx.pack_pcm_device(floats, "PCM_16").cpu().numpy().tobytes()
    full = _wav(res["full_vocal_file"])[4]
    assert full == want
    # .. and the host statement on the first two seconds (outputs whose taps all lie inside the slice): one step at most, rarely
    tpp = -(-Context._resample_filter(160, 147)[0].size // 160)
    n_in = 2 * SR + tpp + 2
    n_chk = (n_in - tpp - 2) * 160 // 147
    host = RE.resample_pack_host(direct["vocal_track_stereo"][:, :n_in], 160, 147, "PCM_16", n_chk).view("<i2").astype(np.int64)
    got = np.frombuffer(full, "<i2")[: n_chk * 2].astype(np.int64)
    assert int(np.max(np.abs(got - host))) <= 1 and np.count_nonzero(got != host) / got.size < SHARE_CAP
    # the vocal segments are its slices at map_cut of the direct run's spans
    spans = _direct_spans(direct)
    assert len(spans) == len(res["vocal_segment_files"])
    ends = []
    for f, (lo, hi) in zip(res["vocal_segment_files"], spans):
        a, b = RE.map_cut(lo, SR, 48000, n_src, n), RE.map_cut(hi, SR, 48000, n_src, n)
        ends += [a, b]
        assert _wav(f)[4] == full[a * 4: b * 4], f
    assert ends[0] == 0 and ends[-1] == n_src and ends[1:-1:2] == ends[2::2]


def test_source_rate_result_and_manifest(runs):
    res, plain, man, direct = runs["res"], runs["plain"], runs["man"], runs["direct"]
    n_src, n = runs["pcm"].shape[0], runs["st44"].shape[1]
    assert res["cut_points_samples"] == plain["cut_points_samples"] == direct["cuts_samples"]
    assert res["sample_rate"] == SR and res["export_sample_rate"] == 48000 and res["source_sample_rate"] == 48000
    assert res["export_cut_points_samples"] == [RE.map_cut(c, SR, 48000, n_src, n) for c in res["cut_points_samples"]]
    assert res["export_cut_points_samples"][0] == 0 and res["export_cut_points_samples"][-1] == n_src
    assert man["export"] == {"sr": 48000, "source_sr": 48000, "cuts_samples": res["export_cut_points_samples"]}
    assert man["audio"]["sr"] == SR and man["cuts"]["samples"] == res["cut_points_samples"]
    on_disk = json.loads((runs["root"] / "source" / "SegmentManifest.json").read_text())
    assert on_disk["export"] == man["export"]
    # the names are those of a run without the setting
    names = lambda r: [f.rsplit("/", 1)[1] for f in r["saved_files"]]
    assert names(res) == names(plain)


def test_without_the_setting_the_files_are_todays(runs):
    plain, plain_man, st44 = runs["plain"], runs["plain_man"], runs["st44"]
    assert "export" not in plain_man and not any(k in plain for k in ("export_sample_rate", "source_sample_rate", "export_cut_points_samples"))
    spans = _direct_spans(runs["direct"])
    mix_bytes, _ = AE.pcm_bytes_host(st44.T, "PCM_16")
    for f, (lo, hi) in zip(plain["mix_segment_files"], spans):
        with open(f, "rb") as fh:
            assert fh.read() == AE.wav_header(hi - lo, SR, 2, 2) + mix_bytes[lo * 4: hi * 4].tobytes(), f
    voc_bytes, _ = AE.pcm_bytes_host(runs["direct"]["vocal_track_stereo"].T, "PCM_16")
    with open(plain["full_vocal_file"], "rb") as fh:
        assert fh.read() == AE.wav_header(st44.shape[1], SR, 2, 2) + voc_bytes.tobytes()


def test_mono_load_at_an_integer_rate(hip_ctx, runs, tmp_path):
    """`audio.channels: 1` and 96 kHz: the file's rate is neither the pipeline's nor the output's, so the stems and the mix all go
    through the kernel (up 320 / down 147) from the resident 44.1 kHz tracks."""
    man = api.separate_and_segment(input_uri=str(runs["src"]), export_dir=str(tmp_path / "out"),
                                   runtime_overrides={"audio.channels": 1, "output.sample_rate": 96000})
    res = api.last_result()
    n = res["cut_points_samples"][-1]
    n_out = -(-n * 320 // 147)
    assert man["export"]["sr"] == 96000 and man["export"]["source_sr"] == 48000 and man["export"]["cuts_samples"][-1] == n_out
    for f in res["saved_files"]:
        ch, width, rate, _, _ = _wav(f)
        assert (ch, width, rate) == (1, 3, 96000), f
    assert _wav(res["full_vocal_file"])[3] == _wav(res["full_instrumental_file"])[3] == n_out
    mix44, file_sr = api.load_audio_device(str(runs["src"]), hip_ctx, 1)
    mix44 = hip_ctx.resample_poly(mix44, SR, file_sr)
    assert mix44.numel() == n
    want = RE.resample_pack_device(hip_ctx, mix44, 320, 147, "PCM_24").cpu().numpy().tobytes()
    assert b"".join(_wav(f)[4] for f in res["mix_segment_files"]) == want and len(want) == n_out * 3
    assert sum(_wav(f)[3] for f in res["vocal_segment_files"]) == n_out


def test_vocal_separation_refuses_another_rate(hip_ctx, runs, tmp_path):
    for value in ("source", 96000):
        with pytest.raises(ValueError, match="vocal_separation") as err:
            api.separate_and_segment(input_uri=str(runs["src"]), export_dir=str(tmp_path / "out"), mode="vocal_separation",
                                     runtime_overrides={"output.sample_rate": value})
        assert "v2.2_mdd" in str(err.value) and "full_vocal" in str(err.value) and "full_instrumental" in str(err.value)
    assert not [p for p in (tmp_path / "out").rglob("*") if p.is_file()]
