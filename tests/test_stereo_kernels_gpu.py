"""True-stereo MDX23 kernels (include/audiocut_hip_stereo.h) against the CPU oracle and against the mono kernels (GPU box only).

The track is a 12.3 s `signals.c2_song(..., stereo=True)`: L and R differ by the generator's 5 % decorrelation."""
import numpy as np
import pytest
import torch

from audio_cut_amd._native import NativeError
from audio_cut_amd.testing import signals
from mdx_refs import restated_stereo_ola as _restated_stereo_ola
from oracle import chunking as OC, separator as OS

pytestmark = pytest.mark.gpu
SR = 44100


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-30, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def stereo():
    return signals.c2_song(12.3, seed=4, stereo=True)


def _tables(hip, ranges, n_items_of):
    cs_l, cl_l, wi_l, base = [], [], [], []
    for (cs, ce, es, ee) in ranges:
        base.append(len(cs_l))
        for k in range(n_items_of(cs, ce)):
            cs_l.append(cs); cl_l.append(ce - cs); wi_l.append(k)
    up = lambda a, t: hip.to_device(np.asarray(a, t))
    return (up(cs_l, np.int64), up(cl_l, np.int64), up(wi_l, np.int32), up(base, np.int32),
            up([r[0] for r in ranges], np.int64), up([r[1] - r[0] for r in ranges], np.int64),
            up([r[2] for r in ranges], np.int64), up([r[3] for r in ranges], np.int64))


def _setup(hip, x):
    ranges = OC.plan_sample_ranges(OC.chunk_plan(x.shape[-1] / SR), SR, x.shape[-1])
    items = {}

    def n_items(cs, ce):
        items[(cs, ce)] = OC.mdx_windows(x[..., cs:ce])
        return items[(cs, ce)][0].shape[0]
    return ranges, _tables(hip, ranges, n_items), items


def test_mdx_stft_stereo_against_oracle(hip_ctx, stereo):
    x = stereo
    ranges, (d_cs, d_cl, d_wi, _, _, _, _, _), items = _setup(hip_ctx, x)
    ref = torch.cat([OS.mdx_stft(items[(cs, ce)][0]) for cs, ce, _, _ in ranges])        # [items, 4, F, T]
    xd = hip_ctx.to_device(x)
    amax = torch.zeros((d_cs.numel(), 256), dtype=torch.float32, device=hip_ctx.device)
    spec = hip_ctx.mdx_stft(xd, d_cs, d_cl, d_wi, amax=amax)
    got = spec.permute(0, 1, 3, 2).cpu().numpy()
    assert _rel(got, ref.numpy()) < 2e-6
    assert not np.array_equal(got[:, 0], got[:, 2])                                       # L and R really differ
    # amax = the maximum |value| over all four channels of each (item, frame), exactly
    assert torch.equal(amax.cpu(), spec.abs().amax(dim=(1, 3)).cpu())
    # L == R: the mono kernel's spectrum and amax, bit for bit
    xm = x[0]
    am_m = torch.zeros_like(amax); am_s = torch.zeros_like(amax)
    mono = hip_ctx.mdx_stft(hip_ctx.to_device(xm), d_cs, d_cl, d_wi, amax=am_m)
    dup = hip_ctx.mdx_stft(hip_ctx.to_device(np.stack([xm, xm])), d_cs, d_cl, d_wi, amax=am_s)
    assert torch.equal(mono, dup) and torch.equal(am_m, am_s)
    # a track is [n] or a contiguous planar [2, n]: anything else is refused
    for bad in (xd.t().contiguous(), xd[:, ::2], torch.stack([xd[0]] * 3)):
        with pytest.raises(NativeError):
            hip_ctx.mdx_stft(bad, d_cs, d_cl, d_wi)


def test_mdx_assemble_ola_stereo_exact(hip_ctx, stereo):
    x = stereo
    ranges, (_, _, _, d_base, d_start, d_len, d_es, d_ee), items = _setup(hip_ctx, x)
    ref_spec = torch.cat([OS.mdx_stft(items[(cs, ce)][0]) for cs, ce, _, _ in ranges])
    g = torch.Generator().manual_seed(0)
    fake = ref_spec * (1.0 + 0.3 * torch.randn(ref_spec.shape, generator=g))             # like the U-Net output: not STFT-consistent
    wave = OS.mdx_istft(fake)
    outs, base, nbs, k0 = [], [], [], 0
    for (cs, ce, es, ee) in ranges:
        batch, st, orig = items[(cs, ce)]
        base.append(k0); nbs.append(batch.shape[0])
        outs.append(OC.mdx_assemble(wave[k0:k0 + batch.shape[0]], st, orig))
        k0 += batch.shape[0]
    ref_v, ref_i = OC.overlap_add(x.shape[1], ranges, outs)
    xd = hip_ctx.to_device(x)
    v, i, vs, is_ = hip_ctx.mdx_assemble_ola(xd, hip_ctx.to_device(wave), d_start, d_len, d_es, d_ee, d_base)
    assert np.array_equal(v.cpu().numpy(), ref_v)
    assert np.array_equal(i.cpu().numpy(), ref_i)
    rv, ri = _restated_stereo_ola(x, wave, ranges, base, nbs)
    assert np.array_equal(vs.cpu().numpy(), rv)
    assert np.array_equal(is_.cpu().numpy(), ri)
    # the stems can be skipped: the mono outputs do not change
    v2, i2, none_v, none_i = hip_ctx.mdx_assemble_ola(xd, hip_ctx.to_device(wave), d_start, d_len, d_es, d_ee, d_base,
                                                       stereo_stems=False)
    assert none_v is None and none_i is None and torch.equal(v, v2) and torch.equal(i, i2)


def test_mdx_chunk_vocal_stereo_exact(hip_ctx, stereo):
    x = stereo
    ranges, (_, _, _, d_base, d_start, d_len, _, _), items = _setup(hip_ctx, x)
    rng = np.random.default_rng(1)
    n_items = sum(items[(cs, ce)][0].shape[0] for cs, ce, _, _ in ranges)
    wave = rng.standard_normal((n_items, 2, OC.ITEM_LEN)).astype(np.float32) * 0.3
    lens = [ce - cs for cs, ce, _, _ in ranges]
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    xd, wd = hip_ctx.to_device(x), hip_ctx.to_device(wave)
    for mix_minus in (False, True):
        got = hip_ctx.mdx_chunk_vocal(xd, wd, d_start, d_len, hip_ctx.to_device(offsets[:-1]), d_base, int(offsets[-1]),
                                      mix_minus=mix_minus).cpu().numpy()
        k0 = 0
        for c, (cs, ce, _, _) in enumerate(ranges):
            batch, st, orig = items[(cs, ce)]
            nb = batch.shape[0]
            voc, inst = OC.mdx_assemble(wave[k0:k0 + nb], st, orig, "instrumental" if mix_minus else "vocal")
            assert np.array_equal(got[offsets[c]:offsets[c + 1]], voc), (c, mix_minus)
            k0 += nb
