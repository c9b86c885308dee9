"""Mode `vocal_separation` on the GPU: k_mdx_assemble_pcm<1|2, PCM_24> (audio_cut_amd/csrc/ac_pack.hip) byte for byte against the kernels
it stands in for and against the oracle, with no U-Net involved, and the mode end to end against a `v2.2_mdd` run of the same
input in the same process.

The kernel's references are the EXISTING kernels, `pack_pcm24(mdx_assemble_ola(...))`, and the oracle's `overlap_add(mdx_assemble(...))`
through `pcm_bytes_host` (for a stereo track the per-channel restatement of tests/mdx_refs.py, which is what
tests/test_mdx_kernels_gpu.py holds the stereo stems to).  Plans: those of tests/test_mdx_kernels_gpu.py (10-fold overlap, empty
effective regions, uncovered samples, two items per chunk, a short last chunk, 1 and 257 samples) and three more, so that n % 4
takes 0, 1, 2 and 3 (the last group of 0 - 3 samples leaves byte by byte), a stereo track has an even and an odd length, one
track of 5 samples is a full group and a partial one, and one has waves of 1.5 standard deviations that drive the conversion
into both clip limits.

Energy partials: the three rows, added in index order, against numpy's float64 sums of squares of the oracle's mono stems and
of the mono mix, within relative n * 2^-53 - the worst-case bound of a float64 sum of n non-negative terms (every square of a
float32 is exact in float64).

End to end the files of the mode must hold the bytes of the `full_vocal_file` / `full_instrumental_file` of a `v2.2_mdd` run: the
U-Net path is deterministic and both go through the same stem arithmetic.  The confidences add the same terms in another
float64 order: |difference| <= 1e-9 (n * 2^-53 < 1e-9 for n <= 8e7, and the estimate is a ratio of such sums clipped to [0, 1])."""
import wave

import numpy as np
import pytest
import torch

import mdx_refs as R
from test_mdx_kernels_gpu import OLA_PLANS, OLA_STEREO
from audio_cut_amd.testing import signals
from audio_cut_amd.utils import audio_export as AE
from oracle import chunking as OC

pytestmark = pytest.mark.gpu

SR = 44100
ITEM = R.ITEM

# (id, samples, chunk_plan arguments, wave scale)
EXTRA = [("mod4_is_2", 258, {}, 0.3), ("five_samples", 5, {}, 0.3), ("clipping", 2 * SR + 3, {}, 1.5)]
CASES = {p[0]: (p[1], p[2], 0.3) for p in OLA_PLANS}
CASES.update({k: (n, args, scale) for k, n, args, scale in EXTRA})
PARAMS = [(k, False) for k in CASES] + [(k, True) for k in OLA_STEREO + [e[0] for e in EXTRA]]


def test_cases_reach_every_tail():
    assert {CASES[k][0] % 4 for k, stereo in PARAMS if not stereo} == {0, 1, 2, 3}
    assert {CASES[k][0] % 2 for k, stereo in PARAMS if stereo} == {0, 1}
    ranges = R.plan_ranges(5)
    assert len(ranges) == 1 and len(R.item_tables(ranges)[0]) == 1              # one chunk, one item


def _interleave(x):
    """planar [2, n] -> frame-interleaved [2 n]; a mono track as it is."""
    return np.ascontiguousarray(x.T).reshape(-1) if x.ndim == 2 else x


@pytest.mark.parametrize("key,stereo", PARAMS)
def test_assemble_pcm24_exact_over_plans(hip_ctx, key, stereo):
    n, args, scale = CASES[key]
    ranges = R.plan_ranges(n, **args)
    c_start, c_len, c_es, c_ee, c_base = R.chunk_tables(ranges)
    n_items = len(R.item_tables(ranges)[0])
    nbs = np.diff(np.append(c_base, n_items)).tolist()
    rng = np.random.default_rng(n + stereo)
    x = (0.3 * rng.standard_normal((2, n) if stereo else n, dtype=np.float32))
    wave_h = rng.standard_normal((n_items, 2, ITEM), dtype=np.float32) * np.float32(scale)
    ch = 2 if stereo else 1

    # the oracle's stems
    outs = []
    for c, (cs, ce, es, ee) in enumerate(ranges):
        batch, aligned, orig = OC.mdx_windows(x[..., cs:ce])
        outs.append(OC.mdx_assemble(wave_h[c_base[c]: c_base[c] + nbs[c]], aligned, orig))
    ref_v, ref_i = OC.overlap_add(n, ranges, outs)
    if ref_i is None:
        ref_i = np.zeros(n, np.float32)
    if stereo:
        o_stem, o_rest = R.restated_stereo_ola(x, wave_h, ranges, c_base.tolist(), nbs)
    else:
        o_stem, o_rest = ref_v, ref_i
    mono_mix = ((x[0] + x[1]) * np.float32(0.5)) if stereo else x

    xd, wd = hip_ctx.to_device(x), hip_ctx.to_device(wave_h)
    tables = [hip_ctx.to_device(a) for a in (c_start, c_len, c_es, c_ee, c_base)]
    stem_d, rest_d, parts_d = hip_ctx.mdx_assemble_pcm24(xd, wd, *tables)
    assert stem_d.dtype == rest_d.dtype == torch.uint8 and stem_d.numel() == rest_d.numel() == 3 * ch * n
    assert parts_d.dtype == torch.float64 and parts_d.shape[0] == 3 and 1 <= parts_d.shape[1] <= 4096
    stem, rest, parts = stem_d.cpu().numpy(), rest_d.cpu().numpy(), parts_d.cpu().numpy()

    # 1. the existing kernels: assemble, (interleave,) pack
    v, i, vs, is_ = hip_ctx.mdx_assemble_ola(xd, wd, *tables)
    k_stem, k_rest = (vs, is_) if stereo else (v, i)
    pack = lambda t: hip_ctx.pack_pcm24(t.t().contiguous().reshape(-1) if stereo else t)
    assert np.array_equal(stem, pack(k_stem)), "stem bytes differ from pack_pcm24(mdx_assemble_ola)"
    assert np.array_equal(rest, pack(k_rest)), "rest bytes differ from pack_pcm24(mdx_assemble_ola)"
    # 2. the oracle through the host conversion
    assert np.array_equal(stem, AE.pcm_bytes_host(_interleave(o_stem), "PCM_24")[0])
    assert np.array_equal(rest, AE.pcm_bytes_host(_interleave(o_rest), "PCM_24")[0])
    # 3. samples that no effective region covers are zero bytes
    uncovered = R.coverage(n, ranges) == 0
    if key in dict((p[0], p) for p in OLA_PLANS):
        assert int(uncovered.sum()) == dict((p[0], p) for p in OLA_PLANS)[key][8]
    for got in (stem, rest):
        assert not got.reshape(n, 3 * ch)[uncovered].any()
    if scale > 1.0:                                                            # both clip limits, in both streams
        words = lambda b: b.reshape(-1, 3).astype(np.int32) @ np.array([1, 256, 65536], np.int32)
        for got in (stem, rest):
            w = words(got)
            assert np.any(w == 0x7FFFFF) and np.any(w == 0x800000)
    # 4. swapped output pointers swap the streams (which stream is the vocal is the caller's choice), and nothing else changes
    from audio_cut_amd._native import _check, _ptr, _stream
    a = torch.empty_like(stem_d); b = torch.empty_like(rest_d); p2 = torch.empty_like(parts_d)
    _check(hip_ctx.lib.ac_mdx_assemble_pcm24(hip_ctx._h, _ptr(xd), n, ch, _ptr(wd), *[_ptr(t) for t in tables], len(ranges), _ptr(b), _ptr(a),
                                             _ptr(p2), parts_d.shape[1], _stream()))
    assert torch.equal(a, rest_d) and torch.equal(b, stem_d) and torch.equal(p2, parts_d)
    # 5. the energy sums
    bound = n * 2.0 ** -53
    for row, ref in zip(parts, (ref_v, ref_i, mono_mix)):
        want = float(np.sum(ref.astype(np.float64) ** 2))
        got = float(np.sum(row))
        print(f"{key} stereo={stereo}: sum of squares {got!r} against {want!r}, relative difference {abs(got - want) / want if want else 0.0:.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound * want
    # one partial row alone, with one workgroup, gives the same sums to the same bound (the grid-stride walk)
    _check(hip_ctx.lib.ac_mdx_assemble_pcm24(hip_ctx._h, _ptr(xd), n, ch, _ptr(wd), *[_ptr(t) for t in tables], len(ranges), _ptr(a), _ptr(b),
                                             _ptr(p2), 1, _stream()))
    assert torch.equal(a, stem_d) and torch.equal(b, rest_d)
    for got, ref in zip(p2.cpu().numpy().reshape(-1)[:3], (ref_v, ref_i, mono_mix)):
        want = float(np.sum(ref.astype(np.float64) ** 2))
        assert abs(float(got) - want) <= bound * want


def test_wrapper_refusals(hip_ctx):
    from audio_cut_amd import _native
    dev = hip_ctx.device
    t = [torch.zeros(1, dtype=torch.int64, device=dev)] * 4 + [torch.zeros(1, dtype=torch.int32, device=dev)]
    w = torch.zeros((1, 2, ITEM), device=dev)
    for bad in (torch.zeros((3, 8), device=dev), torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(0, device=dev)):
        with pytest.raises(_native.NativeError):
            hip_ctx.mdx_assemble_pcm24(bad, w, *t)


@pytest.mark.parametrize("output_type", ["vocal", "instrumental"])
def test_backend_export_path_against_the_float_path(hip_ctx, output_type):
    """`separate_track(export_pcm24=True)` against `separate_track()` of the same backend on a short track: the byte streams are the
    packed float stems and the partial sums the stems' energies, also for an instrumental-type network, whose two streams and
    first two rows of partials change places on the host."""
    from audio_cut_amd import config as cfg
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.utils.gpu_pipeline import ChunkPlan
    saved = cfg.snapshot()
    cfg.set_runtime_config({"enhanced_separation.mdx23.output_type": output_type})
    try:
        backend = MDX23HipBackend(weights=synth_weights(TfcTdfSpec(), seed=0), ctx=hip_ctx)
    finally:
        cfg.restore(saved)
    backend.load_model()
    assert backend.get_output_type() == output_type
    x = signals.c2_song(2.0, seed=3)
    n = x.shape[-1]
    xd = hip_ctx.to_device(x)
    plans = [ChunkPlan(index=0, start_s=0.0, end_s=n / float(SR), halo_left_s=0.0, halo_right_s=0.0)]
    ref = backend.separate_track(xd, SR, plans)
    got = backend.separate_track(xd, SR, plans, export_pcm24=True)
    assert (got.channels, got.n, got.n_items, got.chunk_ranges) == (1, n, ref.n_items, ref.chunk_ranges)
    assert np.array_equal(got.vocal.cpu().numpy(), hip_ctx.pack_pcm24(ref.vocal))
    assert np.array_equal(got.instrumental.cpu().numpy(), hip_ctx.pack_pcm24(ref.instrumental))
    sums = got.energy_partials.cpu().numpy().sum(axis=1)
    for mine, stem in zip(sums, (ref.vocal, ref.instrumental, xd)):
        want = hip_ctx.mean_square(stem) * n
        assert want > 0.0 and abs(float(mine) - want) <= 2.0 * n * 2.0 ** -53 * want       # two float64 sums of the same n terms
    assert not np.array_equal(got.vocal.cpu().numpy(), got.instrumental.cpu().numpy())
    with pytest.raises(ValueError, match="U-Net stream"):
        backend.separate_track(xd, SR, plans, export_pcm24=True, unet_stream=torch.cuda.Stream())


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x):
    pcm = np.clip(np.rint((x.T if x.ndim == 2 else x) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.ndim); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.tobytes())


def _data_chunk(path):
    raw = open(path, "rb").read()
    return raw[:44], raw[44:]


@pytest.mark.parametrize("channels", [1, 2])
def test_mode_writes_the_stems_of_a_v22_run(hip_ctx, tmp_path, channels):
    from audio_cut_amd import api
    song = signals.c2_song(14.0, seed=9, stereo=channels == 2)
    src = tmp_path / "song.wav"
    _write_wav(src, song)
    n = song.shape[-1]
    over = {"audio.channels": 2} if channels == 2 else None
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "sep"), mode="vocal_separation", export_manifest=True,
                                   runtime_overrides=over)
    res = api.last_result()
    assert res["method"] == "vocal_separation_only" and res["num_segments"] == 0 and res["success"] is True
    names = [f"song_vocal_{n / SR:.1f}.wav", f"song_instrumental_{n / SR:.1f}.wav"]
    assert [p.name for p in sorted((tmp_path / "sep").rglob("*.wav"))] == sorted(names)
    assert [res["full_vocal_file"], res["full_instrumental_file"]] == [str(tmp_path / "sep" / f) for f in names] == res["saved_files"]
    assert res["export_plan"] == ["full_instrumental", "full_vocal"] and res["segment_durations"] == []
    assert man["stats"]["num_segments"] == 0 and man["cuts"] == {"final": [], "samples": [], "suppressed": []} and man["segments"] == []
    assert man["artifacts"]["vocal_full"] == names[0] and man["artifacts"]["instrumental_full"] == names[1]
    assert man["audio"]["channels"] == channels and man["gpu"]["gpu_pipeline_used"] is True
    assert res["gpu_pipeline_processed_chunks"] >= 1 and res["gpu_pipeline_compute_ms"] > 0.0

    api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "mdd"), mode="v2.2_mdd",
                             export_types=["full_vocal", "full_instrumental"], runtime_overrides=over)
    ref = api.last_result()
    for kind in ("full_vocal_file", "full_instrumental_file"):
        head, data = _data_chunk(res[kind])
        ref_head, ref_data = _data_chunk(ref[kind])
        assert head == ref_head == AE.wav_header(n, SR, channels, 3)
        assert len(data) == 3 * channels * n and data == ref_data, kind
    print(f"confidence {res['separation_confidence']!r} against {ref['separation_confidence']!r}")
    assert abs(res["separation_confidence"] - ref["separation_confidence"]) <= 1e-9
    assert res["backend_used"] == ref["backend_used"]


def test_mode_with_the_vocal_alone(hip_ctx, tmp_path):
    from audio_cut_amd import api
    song = signals.c2_song(14.0, seed=9)
    src = tmp_path / "song.wav"
    _write_wav(src, song)
    api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), mode="vocal_separation", export_types=["full_vocal"])
    res = api.last_result()
    name = f"song_vocal_{song.shape[-1] / SR:.1f}.wav"
    assert [p.name for p in (tmp_path / "out").rglob("*") if p.is_file()] == [name]
    assert res["saved_files"] == [res["full_vocal_file"]] and res["full_instrumental_file"] is None and res["export_plan"] == ["full_vocal"]
