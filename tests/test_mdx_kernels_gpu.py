"""MDX23 front and back end (audio_cut_amd/csrc/ac_mdx.hip) kernel by kernel: k_mdx_stft<1|2>, k_mdx_istft_frames, k_mdx_istft_ola and
k_mdx_assemble_ola<1|2> against the plain float64 references of tests/mdx_refs.py, which are pinned against torch in float64 on the
CPU first.

Accuracy.  The error of a transform is e = max |got - float64| / scale with the scale a float32 evaluation's error is proportional
to (the windowed frame's L2 norm for the STFT, the overlap-added frame RMS for the iSTFT: mdx_refs.stft_scale / istft_scale), so a
quiet bin or a quiet frame weighs like a loud one.  The yardstick is the same quantity for the oracle's float32 torch.stft /
torch.istft on the same input, and the condition the one of tests/test_unet_gpu.py: e_hip <= 4 * e_f32 + 2**-24.  Both numbers are
printed.  Where the scale is 0 (a frame that holds padding only, a sample no non-zero frame reaches) the kernel must give exactly 0.
The condition is then applied a second time frame by frame (block of 1024 samples by block for a wave), because torch's float32
Hann window is 2.6 % off at its first and last coefficients: a frame that holds one sample under them, or the rim of a lone frame's
support, puts the whole-tensor e_f32 at 1e-2 (on the CPU: 2.6e-2 for a chunk of GEN samples, 6e-2 for a single frame), where the
median frame's is 5e-7.  See `_hold_to_the_yardstick`.

Which test reaches which path:
  k_mdx_stft<1>      noise, loud next to quiet frames, a song, a chunk inside a longer track (win_index 1, audio in the reflected right
                     margin, zeros past chunk_len though the track goes on)                 test_stft_against_float64
                     chunks of 1, 4095, 4096, GEN - 100, GEN, GEN + 1 samples in one launch, frames of padding only
                                                                                           test_stft_chunk_lengths_in_one_launch
                     impulses on chunk sample 0, on item 0's right reflection pivot and on item 1's left one
                                                                                           test_stft_impulses_at_the_reflection_pivots
                     spec_amax (every test above), a silent track                          test_stft_of_silence_is_all_zero
  k_mdx_stft<2>      L != R noise                                                          test_stft_against_float64[stereo_noise]
                     one silent channel against the mono kernel, bit for bit               test_stft_stereo_with_one_silent_channel_is_the_mono_kernel
  n_items refusals                                                                         test_stft_refuses_bad_item_counts, test_istft_refusals
  k_mdx_istft_*      perturbed (not STFT-consistent) spectra                               test_istft_against_float64
                     imaginary part of DC ignored                                          test_istft_ignores_the_imaginary_part_of_dc
                     one non-zero frame: t_lo = 0, the t_hi clamp, the frames where the count of covering frames changes
                                                                                           test_istft_single_frame
                     items in one launch against one launch each                           test_istft_items_are_independent_of_their_batch
                     both transforms in a row                                              test_round_trip_over_the_kept_region
  k_mdx_assemble_ola<1|2>
                     10-fold overlap with and without halo, empty effective regions between non-empty ones, samples no region
                     covers (w_acc == 0), one chunk of two items, a short last chunk, tracks of 1 and 257 samples
                                                                                           test_assemble_ola_exact_over_plans

The round trip is compared with istft64(stft64(x)), not with x: the model drops bin 3072, so the pair returns x less each frame's
Nyquist component (for 0.3 noise about 2e-3 per frame, four orders above float32 rounding).

One-token changes to ac_mdx.hip that this file is written to catch, and the test that is aimed at each:
  reflection `-jj` -> `-jj - 1`                test_stft_impulses_at_the_reflection_pivots, and every STFT accuracy test
  the `q < cl` guard dropped                   test_stft_against_float64[offset_chunk], test_stft_chunk_lengths_in_one_launch,
                                               test_round_trip_over_the_kept_region
  `k == 0 ? 0.f :` removed from the iSTFT load test_istft_ignores_the_imaginary_part_of_dc, test_istft_single_frame
  `t_hi` clamped to MDX_T - 2                  test_istft_single_frame[255] (frame 255 of the two accuracy inputs is silent)
  the `if (w_acc == 0.f)` line removed         test_assemble_ola_exact_over_plans[empty_regions], [gaps]"""
import functools

import numpy as np
import pytest
import torch

import mdx_refs as R
from audio_cut_amd import _native
from audio_cut_amd.testing import signals
from oracle import chunking as OC, separator as OS

SR = 44100
GEN, TRIM, ITEM = R.GEN, R.TRIM, R.ITEM
F32_HALF_ULP = 2.0 ** -24
# a float32 FFT of 6144 points lands some 1e-6 of the frame norm from float64 (measured on the CPU: 7e-7 torch.stft, 1.3e-6
# torch.istft).  A yardstick far above that would make the 4x condition say nothing.
YARDSTICK_CAP = 1e-5


def _admitted(e_f32):
    return 4.0 * e_f32 + F32_HALF_ULP


def _admitted_per_group(q_f32, live):
    """What a group's scaled error may be: 4 * max(the oracle's in that group, the oracle's in the median live group) + 2**-24."""
    return _admitted(np.maximum(q_f32, float(np.median(q_f32[live]))))


def _hold_to_the_yardstick(label, q_hip, q_f32, live, where):
    """The accuracy condition on the whole tensor, as tests/test_unet_gpu.py states it, and then group by group (frames of a spectrum,
    blocks of 1024 samples of a wave; `q_*` are the groups' greatest scaled errors, `live` the groups with a scale above 0).
    The whole-tensor yardstick alone can say nothing: torch builds its Hann window in float32, 2.6 % off at hann[1] = 2.6e-7, so
    one frame that holds a single sample under the window's first or last coefficients, or the rim of a lone frame's support, sets
    e_f32 to 1e-2 for the whole case.  Group by group that stays where it is: a group answers to its own yardstick or to the
    median group's, whichever is larger, and the median must be what a float32 transform delivers."""
    e_hip, e_f32 = float(q_hip.max()), float(q_f32.max())
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(q_hip)), q_hip.shape))
    typical = float(np.median(q_f32[live]))
    print(f"{label}: e_hip {e_hip:.3e} e_f32 {e_f32:.3e} (worst {where} {at}); median group e_hip {float(np.median(q_hip[live])):.3e} "
          f"e_f32 {typical:.3e}")
    assert e_hip <= _admitted(e_f32), (label, e_hip, e_f32, at)
    assert typical < YARDSTICK_CAP, (label, typical)
    over = live & ~(q_hip <= _admitted_per_group(q_f32, live))
    assert not over.any(), (label, [(tuple(int(i) for i in g), float(q_hip[tuple(g)]), float(q_f32[tuple(g)])) for g in np.argwhere(over)[:8]],
                            typical)


# ---------------------------------------------------------------------------------------------------------------------
# case builders (shared by the CPU tests and the GPU tests); references are computed once and left unchanged
# ---------------------------------------------------------------------------------------------------------------------
CHUNK_LENGTHS = [1, 4095, 4096, GEN - 100, GEN, GEN + 1]
STFT_CASES = ["noise", "loud_quiet", "song", "offset_chunk", "stereo_noise"]


def _noise(n, seed, channels=None):
    shape = (n,) if channels is None else (channels, n)
    return (0.3 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _stft_case(name):
    """-> (track float32 [n] or [2, n], [(chunk_start, chunk_len), ...])."""
    if name == "noise":                       # every bin carries energy
        return _noise(GEN, 1), [(0, GEN)]
    if name == "loud_quiet":                  # quiet frames next to loud ones
        x = _noise(GEN, 1)
        x[GEN // 2:] *= np.float32(1e-4)
        return x, [(0, GEN)]
    if name == "song":
        x = signals.c2_song(6.0).astype(np.float32)
        return x, [(0, len(x))]
    if name == "offset_chunk":                # the track goes on, on both sides of the chunk
        return _noise(12345 + GEN + 4096 + 5000, 2), [(12345, GEN + 4096)]
    if name == "stereo_noise":
        return _noise(GEN, 3, channels=2), [(0, GEN)]
    if name == "chunk_lengths":
        return _noise(GEN + 1 + 100 * len(CHUNK_LENGTHS), 4), [(100 * i, cl) for i, cl in enumerate(CHUNK_LENGTHS)]
    if name == "impulses":
        # chunk sample 0 = item 0's sample TRIM; cl - 1 = item 0's sample ITEM - 1, the right reflection pivot;
        # GEN - TRIM = item 1's sample 0, the left reflection pivot
        cs, cl = 5, GEN + TRIM
        x = np.zeros(cs + cl + 9, np.float32)
        x[[cs, cs + cl - 1, cs + GEN - TRIM]] = 1.0
        return x, [(cs, cl)]
    raise KeyError(name)


def _ranges(chunks):
    return [(cs, cs + cl, cs, cs + cl) for cs, cl in chunks]


def _items(track, chunks):
    """The reference's own windowing of every chunk: [items, 2, 261120] float32."""
    return np.concatenate([OC.mdx_windows(track[..., cs:cs + cl])[0] for cs, cl in chunks])


@functools.lru_cache(maxsize=None)
def _stft_reference(name):
    """-> items, stft64, scale [items, 4, 1, 256], the scaled error per item and frame of the oracle's float32 torch.stft."""
    track, chunks = _stft_case(name)
    items = _items(track, chunks)
    assert items.shape[0] == len(R.item_tables(_ranges(chunks))[0])
    ref, scale = R.stft64(items), R.spec_scale(items)
    return items, ref, scale, R.per_frame(R.scaled_errors(OS.mdx_stft(items).numpy(), ref, scale))


@functools.lru_cache(maxsize=None)
def _istft_case(name):
    """A spectrum like a network output, not STFT-consistent: the case's STFT times 1 + 0.3 * randn.  float32 [items, 4, 3072, 256]."""
    ref = _stft_reference(name)[1]
    rng = np.random.default_rng(len(name))
    return (ref * (1.0 + 0.3 * rng.standard_normal(ref.shape))).astype(np.float32)


def _istft_reference(spec):
    """-> istft64, istft_scale, the scaled error per item and block of 1024 samples of the oracle's float32 torch.istft."""
    ref, scale = R.istft64(spec), R.istft_scale(spec)
    return ref, scale, R.per_hop(R.scaled_errors(OS.mdx_istft(torch.from_numpy(spec)), ref, scale))


@functools.lru_cache(maxsize=None)
def _istft_case_reference(name):
    return _istft_reference(_istft_case(name))


SINGLE_FRAMES = [0, 2, 3, 252, 255]


@functools.lru_cache(maxsize=None)
def _single_frame_case(t):
    spec = np.zeros((1, 4, R.F, R.T), np.float32)
    spec[:, :, :, t] = np.random.default_rng(100 + t).standard_normal((1, 4, R.F)).astype(np.float32)
    return spec


# (id, samples, chunk_plan arguments, chunks, items, least fold, greatest fold, empty effective regions, uncovered samples)
OLA_PLANS = [
    ("tenfold_halo", 9 * SR + 77, dict(chunk_s=3.0, overlap_s=2.7, halo_s=0.1), 22, 22, 1, 10, 0, 0),
    ("tenfold_no_halo", 6 * SR + 255, dict(chunk_s=1.0, overlap_s=0.9, halo_s=0.0), 52, 52, 1, 10, 0, 0),
    ("empty_regions", 9 * SR + 77, dict(chunk_s=2.0, overlap_s=0.5, halo_s=1.0), 6, 6, 0, 1, 4, 330750),
    ("gaps", 7 * SR + 1, dict(chunk_s=2.0, overlap_s=0.5, halo_s=0.9), 5, 5, 0, 1, 0, 229320),
    ("one_chunk_two_items", 441000, {}, 1, 2, 1, 1, 0, 0),
    ("short_last_chunk", 441001, {}, 2, 3, 1, 2, 0, 0),
    ("one_sample", 1, {}, 1, 1, 1, 1, 0, 0),
    ("257_samples", 257, {}, 1, 1, 1, 1, 0, 0),
]
OLA_BY_ID = {p[0]: p for p in OLA_PLANS}
OLA_STEREO = ["tenfold_halo", "empty_regions", "one_sample", "257_samples"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the references against the oracle, the plans against what they are here for
# ---------------------------------------------------------------------------------------------------------------------
def test_references_match_the_oracle():
    """stft64 / istft64 against torch.stft / torch.istft run in float64 (the oracle's calls, oracle/separator.py, carried to
    float64) to 1e-12 of the peak; the float32 oracle itself lands where a float32 FFT should; the table builders give what the two
    existing MDX tests build by hand, and one item per `mdx_windows` item."""
    x = _noise(ITEM, 0, channels=2)[None]                                     # [1, 2, 261120]
    win = torch.hann_window(R.N_FFT, periodic=True, dtype=torch.float64)
    s = torch.stft(torch.from_numpy(x).double().reshape(-1, ITEM), n_fft=R.N_FFT, hop_length=R.HOP, window=win, center=True,
                   return_complex=True)
    s = torch.view_as_real(s).permute(0, 3, 1, 2).reshape(-1, 4, R.N_FFT // 2 + 1, R.T)[:, :, :R.F].numpy()
    mine = R.stft64(x)
    assert mine.shape == (1, 4, R.F, R.T) and mine.dtype == np.float64
    assert float(np.max(np.abs(mine - s))) <= 1e-12 * float(np.max(np.abs(s)))
    scale = R.stft_scale(x)
    assert scale.shape == (1, 2, R.T)
    # Parseval on the windowed frame: norm^2 = (|X0|^2 + |X3072|^2 + 2 sum |Xk|^2) / 6144; bin 3072 is the one stft64 drops
    z = np.fft.rfft(R.windowed_frames(x), axis=-1)
    pw = np.abs(z) ** 2
    np.testing.assert_allclose(scale ** 2, (pw[..., 0] + pw[..., -1] + 2.0 * pw[..., 1:-1].sum(-1)) / R.N_FFT, rtol=1e-12)
    e_f32, _ = R.scaled_error(OS.mdx_stft(x).numpy(), mine, R.spec_scale(x))
    assert 0.0 < e_f32 < YARDSTICK_CAP

    rng = np.random.default_rng(1)
    spec = (mine * (1.0 + 0.3 * rng.standard_normal(mine.shape))).astype(np.float32)
    spec[:, [1, 3], 0, :] = rng.standard_normal((1, 2, R.T)).astype(np.float32)        # an imaginary part of DC: both sides drop it
    zc = torch.cat([torch.from_numpy(spec).double(), torch.zeros(1, 4, 1, R.T, dtype=torch.float64)], dim=-2)
    zc = zc.reshape(-1, 2, 2, R.F + 1, R.T).reshape(-1, 2, R.F + 1, R.T)
    zc = torch.view_as_complex(zc.permute(0, 2, 3, 1).contiguous())
    w = torch.istft(zc, n_fft=R.N_FFT, hop_length=R.HOP, window=win, center=True).reshape(-1, 2, ITEM).numpy()
    mine_w = R.istft64(spec)
    assert mine_w.shape == (1, 2, ITEM)
    assert float(np.max(np.abs(mine_w - w))) <= 1e-12 * float(np.max(np.abs(w)))
    iscale = R.istft_scale(spec)
    assert iscale.shape == (1, 2, ITEM) and float(iscale.min()) > 0.0
    e_f32, _ = R.scaled_error(OS.mdx_istft(torch.from_numpy(spec)), mine_w, iscale)
    assert 0.0 < e_f32 < YARDSTICK_CAP
    # the pair gives back x less the dropped bin: with bin 3072 of every frame added again it is x to float64 rounding
    nyq = z[..., -1].real[..., None] / R.N_FFT * np.where(np.arange(R.N_FFT) % 2, -1.0, 1.0)
    back = R.istft64(mine) + R._overlap_add(nyq * R.hann64())
    assert float(np.max(np.abs(back - x))) < 1e-12

    # tables: the loop of tests/test_kernels_gpu.py::test_mdx_stft_istft_assemble, on its own plan and on one with empty regions
    for n, args in ((int(12.3 * SR), {}), (9 * SR + 77, dict(chunk_s=2.0, overlap_s=0.5, halo_s=1.0))):
        ranges = OC.plan_sample_ranges(OC.chunk_plan(n / SR, **args), SR, n)
        assert R.plan_ranges(n, **args) == ranges
        track = np.zeros(n, np.float32)
        cs_l, cl_l, wi_l, base = [], [], [], []
        for (cs, ce, es, ee) in ranges:
            base.append(len(cs_l))
            for k in range(OC.mdx_windows(track[cs:ce])[0].shape[0]):
                cs_l.append(cs); cl_l.append(ce - cs); wi_l.append(k)
        cs_i, cl_i, wi_i = R.item_tables(ranges)
        assert cs_i.dtype == cl_i.dtype == np.int64 and wi_i.dtype == np.int32
        assert (cs_i.tolist(), cl_i.tolist(), wi_i.tolist()) == (cs_l, cl_l, wi_l)
        c_start, c_len, c_es, c_ee, c_base = R.chunk_tables(ranges)
        assert c_base.dtype == np.int32 and c_base.tolist() == base
        assert [(a, a + b, c, d) for a, b, c, d in zip(c_start.tolist(), c_len.tolist(), c_es.tolist(), c_ee.tolist())] == ranges
    for cl in CHUNK_LENGTHS + [GEN + TRIM, GEN + 4096]:
        assert len(R.item_tables([(0, cl, 0, cl)])[0]) == OC.mdx_windows(np.zeros(cl, np.float32))[0].shape[0] == (1 if cl <= 4096 else 2)


def test_plans_have_the_coverage_they_claim():
    """Chunk count, item count, fold and gaps of every overlap-add plan, exactly: a change to the planner cannot quietly turn them
    into the easy case.  eff_start and eff_end ascend in every plan, which is what the kernel's binary search stands on."""
    for key, n, args, chunks, items, fold_lo, fold_hi, empty, uncovered in OLA_PLANS:
        ranges = R.plan_ranges(n, **args)
        cnt = R.coverage(n, ranges)
        c_start, c_len, c_es, c_ee, c_base = R.chunk_tables(ranges)
        got = (len(ranges), len(R.item_tables(ranges)[0]), int(cnt.min()), int(cnt.max()), sum(1 for r in ranges if r[3] <= r[2]),
               int(np.sum(cnt == 0)))
        assert got == (chunks, items, fold_lo, fold_hi, empty, uncovered), key
        assert items <= 52
        assert np.all(np.diff(c_es) >= 0) and np.all(np.diff(c_ee) >= 0), key
        assert np.all(c_es >= c_start) and np.all(c_ee <= c_start + c_len) and np.all(c_start + c_len <= n), key
    ranges = R.plan_ranges(OLA_BY_ID["empty_regions"][1], **OLA_BY_ID["empty_regions"][2])
    empty = [r[3] <= r[2] for r in ranges]
    assert empty == [False, True, True, True, True, False]                    # empty regions BETWEEN non-empty ones
    last = R.plan_ranges(441001)[-1]
    assert last[1] - last[0] == 110251                                        # the 2.5 s last chunk


# ---------------------------------------------------------------------------------------------------------------------
# STFT
# ---------------------------------------------------------------------------------------------------------------------
def _run_stft(hip, track, chunks):
    """-> spectrum [items, 4, 256, 3072] and amax [items, 256] on the device."""
    cs, cl, wi = R.item_tables(_ranges(chunks))
    amax = torch.zeros((len(cs), R.T), dtype=torch.float32, device=hip.device)
    spec = hip.mdx_stft(hip.to_device(track), hip.to_device(cs), hip.to_device(cl), hip.to_device(wi), amax=amax)
    return spec, amax


def _hold_stft_to_float64(hip, name):
    """The accuracy condition, exact zeros where the frame is all padding, and amax; -> the spectrum as [items, 4, 3072, 256]."""
    track, chunks = _stft_case(name)
    items, ref, scale, q_f32 = _stft_reference(name)
    spec, amax = _run_stft(hip, track, chunks)
    assert torch.equal(amax, spec.abs().amax(dim=(1, 3)))                     # max |value| over the four channels and the bins, exactly
    got = spec.permute(0, 1, 3, 2).cpu().numpy()
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    assert not got[np.broadcast_to(scale == 0.0, got.shape)].any(), "a frame of padding only is not exactly zero"
    q = R.scaled_errors(got, ref, scale)
    _, at = R.scaled_error(got, ref, scale)
    print(f"stft {name}: worst at item {at[0]} channel {at[1]} bin {at[2]} frame {at[3]}")
    _hold_to_the_yardstick(f"stft {name}", R.per_frame(q), q_f32, np.any(scale[:, :, 0, :] > 0.0, axis=1), "(item, frame)")
    return got, amax.cpu().numpy(), scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", STFT_CASES)
def test_stft_against_float64(hip_ctx, name):
    got, _, _ = _hold_stft_to_float64(hip_ctx, name)
    if name == "stereo_noise":
        assert not np.array_equal(got[:, 0], got[:, 2])                       # L and R really differ
    else:
        assert np.array_equal(got[:, :2], got[:, 2:])                         # a mono track goes to both channels
    if name == "offset_chunk":
        assert R.item_tables(_ranges(_stft_case(name)[1]))[2].tolist() == [0, 1]


@pytest.mark.gpu
def test_stft_chunk_lengths_in_one_launch(hip_ctx):
    """Six chunks of one track, 1 to GEN + 1 samples: GEN - 100 aligns past GEN, so its second item holds audio in its left trim
    margin only.  Frames whose whole window lies in padding are exactly 0.0 in all four channels, and so is their amax."""
    got, amax, scale = _hold_stft_to_float64(hip_ctx, "chunk_lengths")
    silent = np.all(scale[:, :, 0, :] == 0.0, axis=1)                         # [items, 256]
    assert R.item_tables(_ranges(_stft_case("chunk_lengths")[1]))[2].tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 1]
    assert silent.sum(axis=1).tolist()[:3] == [R.T - 5, R.T - 9, R.T - 9]     # 1 sample: frames 1 .. 5; 4095 / 4096: frames 0 .. 8 (9 is past both)
    assert np.all(silent.sum(axis=1) > 0)
    for item, t in zip(*np.nonzero(silent)):
        assert not got[item, :, :, t].any() and amax[item, t] == 0.0, (item, t)
    assert np.all(amax[~silent] > 0.0)


@pytest.mark.gpu
def test_stft_impulses_at_the_reflection_pivots(hip_ctx):
    """Unit impulses on chunk sample 0, on cl - 1 = item 0's last sample and on GEN - TRIM = item 1's sample 0: a reflection about
    the wrong index, or off by one, doubles or moves an impulse, which noise only blurs."""
    got, _, scale = _hold_stft_to_float64(hip_ctx, "impulses")
    live = np.nonzero(np.any(scale[:, :, 0, :] > 0.0, axis=1))
    # item 0: frames 1 .. 5 (chunk sample 0), 247 .. 251 (item sample GEN = item 1's sample 0; frame 252 meets it at hann[0] = 0),
    # 252 .. 255 (the pivot, sample ITEM - 1: the last coefficient of frame 252; frames 253 .. 255 hold it once, it is its own mirror);
    # item 1: frames 0 .. 2 (sample 0: frame 3 meets it at hann[0] = 0), 3 .. 8 (sample 6143)
    assert sorted(zip(live[0].tolist(), live[1].tolist())) == \
        [(0, t) for t in (1, 2, 3, 4, 5, 247, 248, 249, 250, 251, 252, 253, 254, 255)] + [(1, t) for t in range(9)]


@pytest.mark.gpu
def test_stft_of_silence_is_all_zero(hip_ctx):
    for track in (np.zeros(4097, np.float32), np.zeros((2, 4097), np.float32)):
        spec, amax = _run_stft(hip_ctx, track, [(0, 4097)])
        assert spec.shape == (1, 4, R.T, R.F)
        assert not torch.isnan(spec).any() and not spec.any() and not amax.any()


@pytest.mark.gpu
def test_stft_stereo_with_one_silent_channel_is_the_mono_kernel(hip_ctx):
    """R = 0: channels 0 and 1 are the mono kernel's on L bit for bit, 2 and 3 exactly zero, amax the mono one; then L = 0."""
    track, chunks = _stft_case("offset_chunk")
    mono, amax_m = _run_stft(hip_ctx, track, chunks)
    zero = np.zeros_like(track)
    for live, planar in ((0, np.stack([track, zero])), (1, np.stack([zero, track]))):
        st, amax_s = _run_stft(hip_ctx, planar, chunks)
        assert torch.equal(st[:, 2 * live: 2 * live + 2], mono[:, :2]), live
        assert not st[:, 2 - 2 * live: 4 - 2 * live].any(), live
        assert torch.equal(amax_s, amax_m), live


def _refused_without_a_launch(call, out):
    out.fill_(7.0)
    with pytest.raises(_native.NativeError, match="n_items"):
        _native._check(call())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                           # nothing wrote


@pytest.mark.gpu
def test_stft_refuses_bad_item_counts(hip_ctx):
    """n_items of 0 and 65536 (a grid's y extent ends at 65535) come back through `_check` before any launch: valid pointers, one
    item's tables and buffers, a bad count."""
    from audio_cut_amd._native import _ptr, _stream
    n = 4096
    cs, cl, wi = (hip_ctx.to_device(np.asarray(v, t)) for v, t in (([0], np.int64), ([n], np.int64), ([0], np.int32)))
    out = torch.empty((1, 4, R.T, R.F), dtype=torch.float32, device=hip_ctx.device)
    amax = torch.zeros((1, R.T), dtype=torch.float32, device=hip_ctx.device)
    for fn, track in ((hip_ctx.lib.ac_mdx_stft, hip_ctx.to_device(_noise(n, 5))),
                      (hip_ctx.lib.ac_mdx_stft_stereo, hip_ctx.to_device(_noise(n, 5, channels=2)))):
        for bad in (0, 65536):
            _refused_without_a_launch(lambda: fn(hip_ctx._h, _ptr(track), n, _ptr(cs), _ptr(cl), _ptr(wi), bad, _ptr(out), _ptr(amax),
                                                 _stream()), out)
            assert not amax.any()


# ---------------------------------------------------------------------------------------------------------------------
# iSTFT
# ---------------------------------------------------------------------------------------------------------------------
def _run_istft(hip, spec):
    """spec float32 [items, 4, 3072, 256] on the host -> wave [items, 2, 261120] on the device."""
    return hip.mdx_istft(torch.from_numpy(spec).permute(0, 1, 3, 2).contiguous().to(hip.device))


def _hold_istft_to_float64(hip, label, spec, reference):
    ref, scale, q_f32 = reference
    got = _run_istft(hip, spec).cpu().numpy()
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    assert not got[scale == 0.0].any(), "a sample that no non-zero frame reaches is not exactly zero"
    _, at = R.scaled_error(got, ref, scale)
    print(f"istft {label}: worst at item {at[0]} channel {at[1]} sample {at[2]}")
    _hold_to_the_yardstick(f"istft {label}", R.per_hop(R.scaled_errors(got, ref, scale)), q_f32, R.per_hop(scale) > 0.0, "(item, block of 1024)")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "loud_quiet"])
def test_istft_against_float64(hip_ctx, name):
    _hold_istft_to_float64(hip_ctx, name, _istft_case(name), _istft_case_reference(name))


@pytest.mark.gpu
def test_istft_ignores_the_imaginary_part_of_dc(hip_ctx):
    """Channels 1 and 3, bin 0: whatever stands there, the output is the one for zeros there, bit for bit (a c2r transform)."""
    spec = _istft_case("noise").copy()
    spec[:, [1, 3], 0, :] = 0.0
    clean = _run_istft(hip_ctx, spec)
    spec[:, [1, 3], 0, :] = (50.0 * np.random.default_rng(9).standard_normal((spec.shape[0], 2, R.T))).astype(np.float32)
    assert torch.equal(_run_istft(hip_ctx, spec), clean)


@pytest.mark.gpu
@pytest.mark.parametrize("t", SINGLE_FRAMES)
def test_istft_single_frame(hip_ctx, t):
    """A spectrum that is non-zero in frame t alone: exactly 0.0 outside [1024 t - 3072, 1024 t + 3072), the accuracy condition inside.
    Frames 0 and 255 are t_lo = 0 and the t_hi clamp; 2 is the last frame whose window reaches the padding in front of the item, 3
    the first that lies wholly inside, 252 the last that does."""
    spec = _single_frame_case(t)
    got = _hold_istft_to_float64(hip_ctx, f"frame {t}", spec, _istft_reference(spec))
    lo, hi = max(0, R.HOP * t - TRIM), min(ITEM, R.HOP * t + TRIM)
    assert not got[..., :lo].any() and not got[..., hi:].any()
    assert np.all(np.abs(got[..., lo + 1: hi]).max(axis=-1) > 0.0)


@pytest.mark.gpu
def test_istft_items_are_independent_of_their_batch(hip_ctx):
    spec = np.concatenate([_istft_case("noise"), _istft_case("loud_quiet")[:1]])
    assert spec.shape[0] == 3
    batch = _run_istft(hip_ctx, spec)
    for k in range(3):
        assert torch.equal(_run_istft(hip_ctx, spec[k: k + 1])[0], batch[k]), k


@pytest.mark.gpu
def test_round_trip_over_the_kept_region(hip_ctx):
    """istft(stft(x)) of a two-item chunk over [TRIM, TRIM + GEN) of each item, within the sum of the two stages' bounds:
      stage 1  every bin of frame t is within B1_t * stft_scale_t of stft64; an inverse transform of 6144 points turns bins that are
               each off by at most d (re and im) into samples off by at most sqrt(2) d (the sum of the 6144 magnitudes over 6144),
               and the overlap-add weighs frame t by hann / env like any frame;
      stage 2  the kernel's iSTFT is within B2_b * istft_scale of istft64 on the kernel's own spectrum, b the sample's block of 1024.
    B1_t and B2_b are what `_hold_to_the_yardstick` admits frame by frame and block by block.
    The target is istft64(stft64(x)): x less each frame's dropped bin 3072 (see the file's docstring)."""
    name = "offset_chunk"
    track, chunks = _stft_case(name)
    items, ref_spec, scale, q_f32_stft = _stft_reference(name)
    assert items.shape[0] == 2
    spec, _ = _run_stft(hip_ctx, track, chunks)
    wave = hip_ctx.mdx_istft(spec).cpu().numpy()
    spec_host = np.ascontiguousarray(spec.permute(0, 1, 3, 2).cpu().numpy())
    _, iscale, q_f32_istft = _istft_reference(spec_host)
    b1 = _admitted_per_group(q_f32_stft, np.any(scale[:, :, 0, :] > 0.0, axis=1))         # [items, 256]
    b2 = _admitted_per_group(q_f32_istft, R.per_hop(iscale) > 0.0)                         # [items, 255]
    assert float(np.median(b1)) < _admitted(YARDSTICK_CAP) and float(np.median(b2)) < _admitted(YARDSTICK_CAP)
    target = R.istft64(ref_spec)
    bound = np.sqrt(2.0) * R.ola_of_frame_levels(b1[:, None, :] * R.stft_scale(items)) + np.repeat(b2, R.HOP, axis=1)[:, None, :] * iscale
    kept = slice(TRIM, TRIM + GEN)
    err, bound = np.abs(wave - target)[..., kept], bound[..., kept]
    pos = bound > 0.0
    print(f"round trip: worst error / bound {float(np.max(err[pos] / bound[pos])):.3e}, greatest error {float(err.max()):.3e}, "
          f"bound at most {float(bound.max()):.3e}")
    assert np.isfinite(wave).all() and pos[0].all() and pos.mean() > 0.5
    assert np.all(err <= bound)                                               # exactly 0 where nothing reaches the sample
    # and x itself, once the dropped bin is accounted for: the target differs from x by that bin alone
    assert float(np.max(np.abs(target - items)[..., kept])) < 0.05 * float(np.max(np.abs(items)))


@pytest.mark.gpu
def test_istft_refusals(hip_ctx):
    """The wrapper refuses a trailing shape other than (4, 256, 3072) and float64; ac_mdx_istft refuses 0 and 65536 items."""
    from audio_cut_amd._native import _ptr, _stream
    dev = hip_ctx.device
    for bad in (torch.zeros((1, 4, R.F, R.T), device=dev), torch.zeros((1, 2, R.T, R.F), device=dev), torch.zeros((4, R.T, R.F), device=dev),
                torch.zeros((1, 4, R.T, R.F), dtype=torch.float64, device=dev)):
        with pytest.raises(_native.NativeError):
            hip_ctx.mdx_istft(bad)
    spec = torch.zeros((1, 4, R.T, R.F), dtype=torch.float32, device=dev)
    wave = torch.empty((1, 2, ITEM), dtype=torch.float32, device=dev)
    scratch = torch.empty((2 * R.T * R.N_FFT,), dtype=torch.float32, device=dev)
    for bad in (0, 65536):
        _refused_without_a_launch(lambda: hip_ctx.lib.ac_mdx_istft(hip_ctx._h, _ptr(spec), bad, _ptr(wave), _ptr(scratch), _stream()), wave)


# ---------------------------------------------------------------------------------------------------------------------
# stem assembly + overlap-add
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key,stereo", [(p[0], False) for p in OLA_PLANS] + [(k, True) for k in OLA_STEREO])
def test_assemble_ola_exact_over_plans(hip_ctx, key, stereo):
    """vocal and inst equal `overlap_add(mdx_assemble(...))` element for element on a random track and random waves; a stereo track's
    stems equal the per-channel restatement, and skipping them leaves the mono outputs as they are.  Samples that no effective
    region covers are exactly 0.0."""
    _, n, args = OLA_BY_ID[key][:3]
    ranges = R.plan_ranges(n, **args)
    c_start, c_len, c_es, c_ee, c_base = R.chunk_tables(ranges)
    n_items = len(R.item_tables(ranges)[0])
    nbs = np.diff(np.append(c_base, n_items)).tolist()
    rng = np.random.default_rng(n + stereo)
    x = (0.3 * rng.standard_normal((2, n) if stereo else n, dtype=np.float32))
    wave = rng.standard_normal((n_items, 2, ITEM), dtype=np.float32) * np.float32(0.3)
    outs = []
    for c, (cs, ce, es, ee) in enumerate(ranges):
        batch, aligned, orig = OC.mdx_windows(x[..., cs:ce])
        assert batch.shape[0] == nbs[c]
        outs.append(OC.mdx_assemble(wave[c_base[c]: c_base[c] + nbs[c]], aligned, orig))
    ref_v, ref_i = OC.overlap_add(n, ranges, outs)
    if ref_i is None:
        ref_i = np.zeros(n, np.float32)
    xd, wd = hip_ctx.to_device(x), hip_ctx.to_device(wave)
    tables = [hip_ctx.to_device(a) for a in (c_start, c_len, c_es, c_ee, c_base)]
    v, i, vs, is_ = hip_ctx.mdx_assemble_ola(xd, wd, *tables)
    uncovered = R.coverage(n, ranges) == 0
    assert int(uncovered.sum()) == OLA_BY_ID[key][8]
    vh, ih = v.cpu().numpy(), i.cpu().numpy()
    assert not vh[uncovered].any() and not ih[uncovered].any(), "a sample that no effective region covers is not exactly zero"
    assert np.array_equal(vh, ref_v)
    assert np.array_equal(ih, ref_i)
    if not stereo:
        assert vs is None and is_ is None
        return
    rv, ri = R.restated_stereo_ola(x, wave, ranges, c_base.tolist(), nbs)
    vsh, ish = vs.cpu().numpy(), is_.cpu().numpy()
    assert not vsh[:, uncovered].any() and not ish[:, uncovered].any()
    assert np.array_equal(vsh, rv)
    assert np.array_equal(ish, ri)
    v2, i2, none_v, none_i = hip_ctx.mdx_assemble_ola(xd, wd, *tables, stereo_stems=False)
    assert none_v is None and none_i is None and torch.equal(v, v2) and torch.equal(i, i2)
