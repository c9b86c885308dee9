"""Kernel parity at the edges: the entry points the end-to-end fixtures reach only through a few integer decisions, each against a
float64 reference of the same operation, at the product's parameters plus the shapes where kernels go wrong (segments that touch
sample 0 or n, are empty or shorter than a frame, minima on tile boundaries, clipped windows, ragged chunks, bucket padding, the
one-to-two partial switch, silent frames, track ends).  Every check states its tolerance and why.  GPU box only."""
import inspect

import numpy as np
import pytest
import torch

from audio_cut_amd import _native
from audio_cut_amd.testing import signals
from oracle import chunking as OC, detector as OD, librosa_ops as L, resample as ORS

pytestmark = pytest.mark.gpu
SR = 44100


@pytest.fixture(scope="module")
def track():
    """12 s of C1 bursts (digital silence between them) with a noise floor on the second half: exact-zero frames and ordinary ones."""
    x = signals.c1_sine_silence(12.0, seed=7)
    rng = np.random.default_rng(7)
    h = len(x) // 2
    x[h:] += (1e-3 * rng.standard_normal(len(x) - h)).astype(np.float32)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# segment_frame_rms
# ---------------------------------------------------------------------------------------------------------------------
def _segments(n, frame, hop):
    """Edges: a = 0, b = n, lengths 0, 1, hop - 1, hop, frame - 1, frame, k hop; an empty segment between two non-empty ones;
    overlapping and adjacent segments."""
    segs = [(0, 5 * hop), (0, 0), (17, 17 + 1), (1000, 1000 + hop - 1), (5000, 5000 + hop), (5000 + hop, 5000 + hop + frame - 1),
            (9000, 9000 + frame), (9000 + 3, 9000 + 3), (12000, 12000 + 37 * hop), (12000 + 5, 12000 + 5 + 11 * hop + 1),
            (n - 7 * hop, n), (n - 1, n), (n, n), (n - frame, n), (0, n), (300, 300)]
    return segs


def _rms_ref_uncentred(x, a, b, win):
    """oracle/vad.py:energy_probs framing: windows from the segment start, the last one zero-padded."""
    seg = x[a:b]
    nw = (len(seg) + win - 1) // win
    padded = np.zeros(nw * win, dtype=np.float32)
    padded[:len(seg)] = seg
    return np.sqrt(np.mean(np.square(padded.reshape(nw, win).astype(np.float64)), axis=1)).astype(np.float32)


@pytest.mark.parametrize("frame,hop,center", [(2205, 882, True), (4410, 2205, True), (1411, 1411, False)])
def test_segment_frame_rms_edges(hip_ctx, track, frame, hop, center):
    """Classifier (2205 / 882, centred), feature-cache chunk RMS (4410 / 2205, centred) and chunked VAD (1411 / 1411, not centred).
    Centred: librosa.feature.rms of the segment alone at rtol 2e-6 (the `test_frame_rms` precedent: both sum in float64 and
    round once to float32, in different orders), and bit-identical to `frame_rms` of the slice (features_cache.py relies on
    that).  Not centred: energy_probs' framing at the same tolerance.  Exact-zero frames stay exact zeros.  The list repeats the
    whole track until it holds more than 65 535 frames (frame indices and the frame -> segment binary search past 16 bits).
    Regression: with an odd frame (the classifier's 2205) and a segment of a whole number of hops, the wrapper counted
    1 + len // hop frames where librosa has 1 + (len - 1) // hop: one extra frame, centred on the segment's end, entered the
    classifier's activity ratio."""
    n = len(track)
    xd = hip_ctx.to_device(track)
    segs = _segments(n, frame, hop)
    per_full = (n // hop) + 1
    segs += [(0, n)] * (65536 // per_full + 1)
    a = np.array([s[0] for s in segs], np.int64); b = np.array([s[1] for s in segs], np.int64)
    got = hip_ctx.segment_frame_rms(xd, a, b, frame, hop, center=center)
    assert sum(len(g) for g in got) > 65535
    cache = {}
    for (sa, sb), g in zip(segs, got):
        if (sa, sb) not in cache:
            if not center:
                cache[(sa, sb)] = _rms_ref_uncentred(track, sa, sb, frame)
            elif sb - sa + 2 * (frame // 2) < frame:
                cache[(sa, sb)] = np.zeros(0, np.float32)       # librosa raises: no frame fits; the product skips such segments
            else:
                cache[(sa, sb)] = L.rms(track[sa:sb], frame_length=frame, hop_length=hop)[0]
        ref = cache[(sa, sb)]
        assert g.shape == ref.shape, (sa, sb, g.shape, ref.shape)
        np.testing.assert_allclose(g, ref, rtol=2e-6, atol=1e-9, err_msg=str((sa, sb)))
        assert np.array_equal(g == 0.0, ref == 0.0), (sa, sb)
        if center and sb > sa:
            want = hip_ctx.frame_rms(xd[sa:sb], frame, hop).cpu().numpy()
            assert np.array_equal(g, want), (sa, sb)
    assert hip_ctx.segment_frame_rms(xd, np.zeros(0, np.int64), np.zeros(0, np.int64), frame, hop, center=center) == []


# ---------------------------------------------------------------------------------------------------------------------
# segment_sumsq_peak
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_sumsq_peak_edges(hip_ctx, track):
    """Sum of squares against the float64 sum at rtol 1e-12 (float64 accumulation of float32 squares, only the order differs);
    peak exactly max |x| (a max is exact).  Lengths 0, 1 .. 17 (fewer samples than the 16 parts), 4095 and the whole track; a
    segment ending at n and an all-zero one.  The host adds the 16 partials in index order: the total must be THAT sum of the
    kernel's own partials, bit for bit, and two calls must give equal bits."""
    n = len(track)
    zero_at = int(np.flatnonzero(track == 0)[0])
    assert np.all(track[zero_at: zero_at + 40] == 0)
    segs = [(100, 100 + k) for k in range(18)] + [(n - 4095, n), (0, 4095), (0, n), (n, n), (n - 1, n), (zero_at, zero_at + 40), (3, 3 + 31)]
    a = np.array([s[0] for s in segs], np.int64); b = np.array([s[1] for s in segs], np.int64)
    xd = hip_ctx.to_device(track)
    ss, pk = hip_ctx.segment_sumsq_peak(xd, a, b)
    for q, (sa, sb) in enumerate(segs):
        seg = track[sa:sb]
        want = float(np.sum(seg.astype(np.float64) ** 2))
        assert ss[q] == pytest.approx(want, rel=1e-12, abs=0), (sa, sb)
        assert pk[q] == (np.max(np.abs(seg)) if seg.size else 0.0), (sa, sb)
    ss2, pk2 = hip_ctx.segment_sumsq_peak(xd, a, b)
    assert np.array_equal(ss.view(np.int64), ss2.view(np.int64)) and np.array_equal(pk, pk2)
    # the partials: part p owns the p-th contiguous sixteenth; the total is their index-order sum
    da, db_ = hip_ctx.to_device(a), hip_ctx.to_device(b)
    parts = torch.empty((len(segs), 16), dtype=torch.float64, device=hip_ctx.device)
    ppk = torch.empty((len(segs), 16), dtype=torch.float32, device=hip_ctx.device)
    from audio_cut_amd._native import _check, _ptr, _stream
    _check(hip_ctx.lib.ac_segment_sumsq_peak(hip_ctx._h, _ptr(xd), n, _ptr(da), _ptr(db_), len(segs), _ptr(parts), _ptr(ppk), _stream()))
    parts = parts.cpu().numpy()
    for q, (sa, sb) in enumerate(segs):
        total = 0.0
        for p in range(16):
            total += parts[q, p]
        assert total == ss[q], (sa, sb)
        chunk = (sb - sa + 15) // 16
        for p in range(16):
            lo = min(sb, sa + p * chunk); hi = min(sb, lo + chunk)
            assert parts[q, p] == pytest.approx(float(np.sum(track[lo:hi].astype(np.float64) ** 2)), rel=1e-12, abs=0)


# ---------------------------------------------------------------------------------------------------------------------
# local_valley
# ---------------------------------------------------------------------------------------------------------------------
def _valley_ref(x, c, radius, win):
    """The float64 inner loop of oracle/layout.py:refine_local_valley -> (orig_db, min_db, first argmin, db series)."""
    a = max(0, c - radius); b = min(len(x), c + radius)
    seg = x[a:b]
    if seg.size <= win:
        return 0.0, 0.0, -1, None
    sq = np.square(seg.astype(np.float64))
    rms = np.sqrt(np.convolve(sq, np.ones(win, dtype=np.float64) / float(win), mode="valid") + 1e-12)
    db = 20.0 * np.log10(rms + 1e-12)
    o = int(np.clip(c - a - win // 2, 0, db.size - 1))
    v = int(np.argmin(db))
    return float(db[o]), float(db[v]), v, db


def _check_valley(hip_ctx, x, centers, radius, win, exact_idx=()):
    """orig / min dB within 1e-9 dB (float64 window sums in another order); min_idx exact, or a tie within 1e-9 dB: the same rule
    and reason as `test_window_argmin_zero_cross_and_slow_guard` (equal minima are equivalent for refine_local_valley, which uses
    only db[o] - db[v]).  Centres in `exact_idx` must give the exact first index (ties between bit-identical values)."""
    od, md, mi = hip_ctx.local_valley(hip_ctx.to_device(x), np.asarray(centers, np.int64), radius, win)
    for q, c in enumerate(centers):
        o, m, v, db = _valley_ref(x, int(c), radius, win)
        if db is None:
            assert (od[q], md[q], mi[q]) == (0.0, 0.0, -1), (c, od[q], md[q], mi[q])
            continue
        assert abs(od[q] - o) < 1e-9 and abs(md[q] - m) < 1e-9, (c, od[q], o, md[q], m)
        if c in exact_idx:
            assert mi[q] == v, (c, mi[q], v)
        else:
            assert mi[q] == v or abs(db[mi[q]] - db[v]) < 1e-9, (c, mi[q], v)
    return od, md, mi


def test_local_valley_edges(hip_ctx, track):
    """ac_local_valley against the float64 loop of refine_local_valley: the product's radius 8820 / win 882 at centres 0, inside
    one radius of either end and n; a track shorter than `win` and clipped windows of size <= win ((0, 0, -1)); a strict minimum
    on output 1023 and on output 1024 (the last of the first 1024-output tile, the first of the second) and a digitally silent run
    across that tile boundary (bit-identical dB values: the first index must win); win 1 and 2048 accepted, 2049 rejected."""
    n = len(track)
    radius, win = 8820, 882
    centers = [0, 5, radius - 1, radius, 50000, 123457, n - radius, n - radius + 1, n - 3, n]
    _check_valley(hip_ctx, track, centers, radius, win)
    # tracks shorter than win, and clipped windows of exactly win / win + 1 samples
    short = track[:500].copy() + np.float32(0.01)
    _check_valley(hip_ctx, short, [0, 250, 500], radius, win)
    _check_valley(hip_ctx, track[:win + 1].copy(), [0, win // 2, win + 1], radius, win)
    _check_valley(hip_ctx, track[:win].copy(), [0, win // 2, win], radius, win)
    _check_valley(hip_ctx, track, [5000, n // 2], win // 2, win)          # 2 radius == win: never longer than win
    # minimum on output 1023 / 1024 of the window starting at a = c - radius
    rng = np.random.default_rng(3)
    base = (0.3 + 0.01 * rng.standard_normal(60000)).astype(np.float32)
    c = 30000
    a = c - radius
    for out_idx in (1023, 1024, 1022, 2047, 2048):
        x = base.copy()
        x[a + out_idx: a + out_idx + win] *= np.float32(0.01)          # the window over exactly these samples is the quietest
        _, _, mi = _check_valley(hip_ctx, x, [c], radius, win, exact_idx=(c,))
        assert mi[0] == out_idx
    # a silent run across the tile boundary: every window inside it has the same dB bits; the first must win
    x = base.copy()
    x[a + 1000: a + 1000 + win + 60] = 0.0
    _, _, mi = _check_valley(hip_ctx, x, [c], radius, win, exact_idx=(c,))
    assert mi[0] == 1000
    x = base.copy()
    x[a + 2040: a + 2040 + win + 30] = 0.0                              # silent windows 2040 .. 2070: across the 2048 boundary
    _, _, mi = _check_valley(hip_ctx, x, [c], radius, win, exact_idx=(c,))
    assert mi[0] == 2040
    # window sizes: 1 and the LDS limit 2048 work, 2049 is refused before launch
    _check_valley(hip_ctx, track, [0, 40000, n], 3000, 1)
    _check_valley(hip_ctx, track, [0, 40000, n - 100], 3000, 2048)
    with pytest.raises(_native.NativeError):
        hip_ctx.local_valley(hip_ctx.to_device(track), np.array([40000]), 3000, 2049)


# ---------------------------------------------------------------------------------------------------------------------
# resample_poly_segments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", [(160, 441), (3, 2), (7, 7)])
def test_resample_poly_segments_edges(hip_ctx, track, up, down):
    """Every segment is `resample_poly` of the segment alone, bit for bit (ac_polyphase.hip: scipy.signal.resample_poly on the segment
    alone), and within 2e-6 of the float64 oracle (the float32 polyphase dot against float64 scipy: the precedent of
    `test_resample_poly_kernel_vs_oracle`); bucket padding is exactly 0.0.  Lengths 0, 1, 2, 159, 160, 441, 442 and one whose output
    is an exact multiple of the 4096 bucket; buckets 0 and 4096; up == down (a copy).  The 2e-6 covers only the filter DESIGN
    difference with the oracle; the arithmetic is held by the same-taps tests of test_resample_pcm_edges_gpu.py."""
    import math
    g = math.gcd(up, down); u, d = up // g, down // g
    n = len(track)
    exact = (4096 * 3 * d) // u if u != d else 4096 * 3       # output length 3 * 4096 exactly (160 / 441: 33868 samples)
    lens = [0, 1, 2, 159, 160, 441, 442, exact, 20000, 0, 1000]
    offs = [0, 5, n - 2, 777, 1234, 44100, 2 * SR + 17, 3 * SR, n - 20000, n, 96000]
    assert all(o + k <= n for o, k in zip(offs, lens))
    xd = hip_ctx.to_device(track)
    peak = float(np.max(np.abs(track)))
    for bucket in (0, 4096):
        out, out_off, out_len = hip_ctx.resample_poly_segments(xd, offs, lens, up, down, bucket=bucket)
        host = out.cpu().numpy()
        assert out_len[lens.index(exact)] == (3 * 4096 if u != d else exact)
        end = 0
        for o, k, oo, ol in zip(offs, lens, out_off, out_len):
            oo = int(oo)
            assert oo == end
            seg = host[oo: oo + ol]
            if k > 0:
                alone = hip_ctx.resample_poly(xd[o: o + k], up, down).cpu().numpy()
                assert np.array_equal(seg, alone), (o, k, bucket)
                ref = ORS.resample(track[o: o + k], up, down)
                assert seg.shape == ref.shape
                assert float(np.max(np.abs(seg - ref))) <= 2e-6 * max(peak, 1e-30), (o, k)
            else:
                assert ol == 0
            padded = ol + ((-ol) % bucket if bucket else 0)
            assert np.all(host[oo + ol: oo + padded] == 0.0) and not np.any(np.signbit(host[oo + ol: oo + padded]))
            end = oo + padded
        assert end == len(host)
    out, _, out_len = hip_ctx.resample_poly_segments(xd, [0, 10], [0, 0], up, down, bucket=4096)
    assert out.numel() == 0 and out_len == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# mdx_chunk_vocal
# ---------------------------------------------------------------------------------------------------------------------
def test_mdx_chunk_vocal_edges(hip_ctx):
    """The per-chunk mono vocal against a host restatement (item = base + q // GEN, pos = TRIM + q % GEN, (w0 + w1) * 0.5 in
    float32) and against the channel mean of oracle/chunking.mdx_assemble, both EXACT (one float32 add and an exact halving):
    a chunk shorter than one item, exactly one item (GEN samples), one more, a ragged last chunk, and a C5-sized plan (240 chunks)."""
    from audio_cut_amd.separation.backends import items_per_chunk
    from audio_cut_amd.utils.gpu_pipeline import chunk_schedule
    GEN, TRIM, ITEM = OC.GEN, OC.TRIM, OC.ITEM_LEN
    plans = chunk_schedule(1800.0)
    c5 = [int(round(p.end_s * SR)) - int(round(p.start_s * SR)) for p in plans]
    assert len(c5) == 240
    for lens in ([1000, GEN, GEN + 1, 2 * GEN - 5, 3 * GEN + 4096 * 7 + 11, 4095], c5):
        n_it = [items_per_chunk(cl, 4096) for cl in lens]
        base = np.concatenate(([0], np.cumsum(n_it)[:-1])).astype(np.int32)
        offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        gen = torch.Generator(device=hip_ctx.device).manual_seed(11)
        wave = torch.randn((int(sum(n_it)), 2, ITEM), generator=gen, device=hip_ctx.device)
        track = torch.zeros(int(offsets[-1]), dtype=torch.float32, device=hip_ctx.device)    # chunks back to back; never read
        args = (track, wave, hip_ctx.to_device(offsets[:-1].copy()), hip_ctx.to_device(np.asarray(lens, np.int64)),
                hip_ctx.to_device(offsets[:-1].copy()), hip_ctx.to_device(base), int(offsets[-1]))
        got = hip_ctx.mdx_chunk_vocal(*args).cpu().numpy()
        with pytest.raises(_native.NativeError):      # the mono entry point has no mix-minus form
            hip_ctx.mdx_chunk_vocal(*args, mix_minus=True)
        w = wave.cpu().numpy()
        for c, cl in enumerate(lens):
            q = np.arange(cl)
            item = base[c] + q // GEN
            pos = TRIM + q % GEN
            want = (w[item, 0, pos] + w[item, 1, pos]) * np.float32(0.5)
            seg = got[offsets[c]: offsets[c + 1]]
            assert want.dtype == np.float32 and np.array_equal(seg, want), c
            if c < 8 or c == len(lens) - 1:
                aligned = cl + (-cl) % 4096
                vocal, _ = OC.mdx_assemble(w[base[c]: base[c] + n_it[c]], np.zeros((2, aligned), np.float32), cl)
                assert np.array_equal(seg, vocal), c
        del wave, w, track


# ---------------------------------------------------------------------------------------------------------------------
# mean_square / ac_sum_squares
# ---------------------------------------------------------------------------------------------------------------------
def test_mean_square_partials_edges(hip_ctx):
    """mean_square against the float64 mean at rtol 1e-12 (float64 accumulation; only the order differs) across the switch from one
    partial to two at 8192 samples, the 1024-partial cap at 4096 * 1024 and a 30-min track; deterministic bits; ac_sum_squares
    refuses 0 and 4097 partials before launch."""
    rng = np.random.default_rng(13)
    big = (rng.standard_normal(1800 * SR) * 0.2).astype(np.float32)
    xd = hip_ctx.to_device(big)
    for n in (1, 2, 255, 256, 257, 4095, 4096, 8191, 8192, 8193, 4096 * 1024 - 1, 4096 * 1024, 4096 * 1024 + 1, 1800 * SR):
        parts = hip_ctx.sum_squares_parts(xd[:n])
        assert parts.numel() == min(1024, max(1, n // 4096)), n
        got = hip_ctx.mean_square(xd[:n])
        want = float(np.sum(big[:n].astype(np.float64) ** 2)) / n
        assert got == pytest.approx(want, rel=1e-12, abs=0), n
        assert hip_ctx.mean_square(xd[:n]) == got, n
    from audio_cut_amd._native import _check, _ptr, _stream
    buf = torch.empty(4097, dtype=torch.float64, device=hip_ctx.device)
    for bad in (0, 4097):
        with pytest.raises(_native.NativeError):
            _check(hip_ctx.lib.ac_sum_squares(hip_ctx._h, _ptr(xd), 1 << 20, _ptr(buf), bad, _stream()))


# ---------------------------------------------------------------------------------------------------------------------
# dormant multi-feature branch kernels at their edges
# ---------------------------------------------------------------------------------------------------------------------
def _edge_signal(n, seed):
    """Noise with a run of exact zeros, a run of digital silence at the end, and a tone."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = (0.3 * np.sin(2 * np.pi * 310.0 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    x[n // 3: n // 3 + 5000] = 0.0
    x[-3000:] = 0.0
    return x


def test_stft2048_spectral_edges(hip_ctx):
    """Centroid against librosa's spectral_centroid and the low-third ratio against `_calculate_harmonic_ratio_direct` (oracle) at the
    tolerances of `test_dormant_multifeature_branch_against_oracle_and_golden` (float64 FFT vs numpy's, float32 magnitudes):
    silent frames (the len_eff guard: exactly 0 Hz), the first and last frames, n < 2048, n not a multiple of the hop."""
    hop = 441
    for n in (100, 2047, 2048, 441 * 20, 441 * 20 + 17, 3 * SR + 5):
        x = _edge_signal(n, n) if n > 8000 else (0.2 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
        cen, rat = hip_ctx.stft2048_spectral(hip_ctx.to_device(x), SR, hop)
        rc = L.spectral_centroid(x, sr=SR, hop_length=hop)[0]
        rr = OD.harmonic_ratio_direct(x, hop)
        assert cen.shape == rc.shape and rat.shape == rr.shape, n
        np.testing.assert_allclose(cen, rc, rtol=1e-4, atol=1e-2, err_msg=str(n))
        np.testing.assert_allclose(rat, rr, rtol=1e-4, atol=1e-6, err_msg=str(n))
        assert np.array_equal(cen == 0.0, rc == 0.0), n
    z = np.zeros(5000, np.float32)
    cen, rat = hip_ctx.stft2048_spectral(hip_ctx.to_device(z), SR, hop)
    assert np.all(cen == 0.0) and np.all(rat == 0.0)


def test_zero_crossing_rate_edges(hip_ctx):
    """Exact against librosa.feature.zero_crossing_rate (a count over frame_len is exact): samples at +-1e-10 (on the threshold: clipped
    to +0), -0.0 (sign bit set, clipped to +0 as well), runs of exact zeros, n < frame_len / 2 (every frame is edge padding), and an
    odd frame_len, with n that the hop divides and n that it does not.
    Regression: with an odd frame_len librosa has 1 + (n - 1) // hop frames; the wrapper (and the ABI's size check) asked for
    1 + n // hop, one frame too many whenever the hop divides n.  Both now use librosa's count (the product passes 2048)."""
    rng = np.random.default_rng(21)
    n = 30000
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    x[1000:1200] = np.float32(1e-10) * np.where(np.arange(200) % 2 == 0, 1, -1).astype(np.float32)
    x[1200:1300] = np.float32(-0.0)
    x[2000:2600] = 0.0
    x[3000:3100] = np.where(np.arange(100) % 3 == 0, np.float32(-1e-10), np.float32(2e-10))
    x[3100:3200] = np.where(np.arange(100) % 2 == 0, np.float32(-0.0), np.float32(-1e-10))
    x[4000:4100] = np.nextafter(np.float32(1e-10), np.float32(1)) * np.where(np.arange(100) % 2 == 0, 1, -1).astype(np.float32)
    for frame_len, hop, m in ((2048, 441, n), (2048, 441, 441 * 40), (2048, 441, 700), (2048, 441, 1), (2047, 441, n), (2047, 441, 441 * 40), (301, 100, 9999), (301, 100, 10000),
                              (2, 1, 500)):
        y = x[:m]
        got = hip_ctx.zero_crossing_rate(hip_ctx.to_device(y), frame_len, hop)
        ref = L.zero_crossing_rate(y, frame_length=frame_len, hop_length=hop)[0]
        assert got.shape == ref.shape, (frame_len, hop, m)
        assert np.array_equal(got, ref), (frame_len, hop, m)


def test_lpc_formants_edges(hip_ctx):
    """Per-frame LPC peaks against oracle/detector.extract_formants' arithmetic (librosa.lpc + freqz + find_peaks): peak counts
    exact, magnitudes at rtol 5e-3 (the float32 Burg recursion near a pole, the existing precedent); frames of exact zeros (a flat
    |1/A| = 1: no peak); an n with n - frame_len a multiple of the hop (the reference's range() stops one frame early) and one
    frame past it."""
    import scipy.signal as signal
    frame_len, hop = int(0.025 * SR), 441
    base = signals.voice_with_rests(2.0, seed=4)
    base[20000:24000] = 0.0
    for n in (frame_len + 1, frame_len + 5 * hop, frame_len + 5 * hop + 1, len(base)):
        x = base[:n]
        cnt, mag = hip_ctx.lpc_formants(hip_ctx.to_device(x), frame_len, hop, order=12, preemph=0.95)
        starts = list(range(0, n - frame_len, hop))
        assert len(cnt) == len(starts), n
        for f, i in enumerate(starts):
            fr = x[i:i + frame_len]
            fr = np.append(fr[0], fr[1:] - 0.95 * fr[:-1])
            a = L.lpc(fr, 12)
            _, h = signal.freqz(1, a, worN=512, fs=SR)
            m = np.abs(h)
            peaks, _ = signal.find_peaks(m, height=np.max(m) * 0.1)
            assert cnt[f] == len(peaks), (n, f)
            k = min(3, len(peaks))
            np.testing.assert_allclose(mag[f, :k], m[peaks[:k]], rtol=5e-3, atol=1e-6, err_msg=str((n, f)))
            assert np.all(mag[f, k:] == 0.0)
        if n == len(base):
            silent = [f for f, i in enumerate(starts) if np.all(x[i:i + frame_len] == 0)]
            assert silent and np.all(cnt[silent] == 0)


def test_pyin_edges(hip_ctx):
    """ac_yin_f0 -> ac_pyin_observe -> ac_pyin_viterbi against librosa.pyin (oracle): voiced flags and pitch states exact (f0 at rtol
    1e-12: the same bin or a visibly different one), voiced_prob at rtol 1e-9 (float64 throughout, the dormant-branch precedent);
    silence, tracks of one and two frames, a glide across many bins, and a jump far outside the transition band (200 -> 300 Hz:
    70 bins against a 41-bin band; librosa's path crosses it through unvoiced states, and k_pyin_viterbi weighs the out-of-band
    `global max + log(tiny)` predecessor at every step of it)."""
    fmin, fmax = 65.40639132514966, 2093.004522404789
    rng = np.random.default_rng(8)
    t = np.arange(int(1.5 * SR)) / SR
    glide_f = 110.0 * 2.0 ** (2.5 * t / t[-1])
    glide = (0.5 * np.sin(2 * np.pi * np.cumsum(glide_f) / SR)).astype(np.float32)
    jump_f = np.where(t < 0.75, 200.0, 300.0)
    jump = (0.5 * np.sin(2 * np.pi * np.cumsum(jump_f) / SR) + 0.001 * rng.standard_normal(len(t))).astype(np.float32)
    cases = {"silence": np.zeros(8192, np.float32), "one_frame": (0.2 * rng.standard_normal(300)).astype(np.float32),
             "two_frames": (0.2 * rng.standard_normal(500)).astype(np.float32), "glide": glide, "jump": jump}
    for name, x in cases.items():
        f0, voiced, vp = hip_ctx.pyin(hip_ctx.to_device(x), SR, fmin, fmax, frame_length=2048, hop=441)
        rf0, rv, rvp = L.pyin(x, fmin, fmax, sr=SR, frame_length=2048, hop_length=441)
        assert f0.shape == rf0.shape, name
        assert np.array_equal(voiced, rv), name
        assert np.array_equal(np.isnan(f0), np.isnan(rf0)), name
        v = ~np.isnan(rf0)
        np.testing.assert_allclose(f0[v], rf0[v], rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(vp, rvp, rtol=1e-9, atol=1e-12, err_msg=name)
        if name == "glide":
            assert v.sum() > 100 and np.nanmax(rf0) / np.nanmin(rf0) > 4.0
        if name == "jump":
            ft = np.arange(len(rf0)) * 441 / SR
            assert np.all(np.abs(rf0[(ft < 0.6) & v] - 200) < 5) and np.all(np.abs(rf0[(ft > 0.9) & v] - 300) < 5)


# ---------------------------------------------------------------------------------------------------------------------
# the U-Net at the shipped batch size
# ---------------------------------------------------------------------------------------------------------------------
def test_separation_is_independent_of_items_per_forward(hip_ctx):
    """The library default items per forward (read from the signature), 32 (what every oracle-fixture test pins) and 7 give the same
    bits: vocal, instrumental and the per-chunk VAD input, on the 240 s C2 track of the `c2_full_oracle` fixture and on a C5 plan
    (480 items: 7 x 64 + 32 at the default).  At 64 items the level-0 activations hold 2.4e9 elements (more than 2^31), so a 32-bit
    offset anywhere in the U-Net kernels would show here; the fixtures at 32 then carry over to the default."""
    from audio_cut_amd.separation.backends import MDX23HipBackend
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    from audio_cut_amd.utils.gpu_pipeline import chunk_schedule
    default = inspect.signature(MDX23HipBackend.__init__).parameters["max_items_per_forward"].default
    assert default > 32
    weights = synth_weights(TfcTdfSpec(), seed=0)
    backends = {k: MDX23HipBackend(weights=weights, ctx=hip_ctx, max_items_per_forward=k) for k in (default, 32, 7)}
    for backend in backends.values():
        backend.load_model()
    for mix, n_items in ((signals.c2_song(240.0, seed=2), None), (signals.c5_long_form(1800.0, seed=5), 480)):
        dev = hip_ctx.to_device(mix)
        plans = chunk_schedule(len(mix) / SR)
        first = None
        for k, backend in backends.items():
            sep = backend.separate_track(dev, SR, plans)
            if n_items is not None:
                assert sep.n_items == n_items
            if first is None:
                first = sep
                continue
            assert torch.equal(sep.vocal, first.vocal), (len(mix), k)
            assert torch.equal(sep.instrumental, first.instrumental), (len(mix), k)
            assert torch.equal(sep.chunk_vocal, first.chunk_vocal), (len(mix), k)
            del sep
        print(f"{len(mix) / SR:.0f} s, {first.n_items} items: items per forward {default} / 32 / 7 bit-identical")
        del first, dev
        torch.cuda.empty_cache()


def test_level0_conv_at_64_items_matches_2_items(hip_ctx):
    """The level-0 3x3 conv (conv3x3_f16x3_s8, 48 -> 48, 256 x 3072) at B = 64: 2.4e9 elements per tensor, so items 57 .. 63 lie
    beyond 2^31.  Items 0, 31, 32 and 63 must equal, bit for bit, the same items run at B = 2 (a per-item computation whose offsets
    are 64-bit)."""
    from audio_cut_amd.separation.conv_pack import pack_conv3x3_w96
    dev = hip_ctx.device
    gen = torch.Generator(device=dev).manual_seed(64)
    x = torch.randn((64, 48, 256, 3072), generator=gen, device=dev)
    assert x.numel() > 2 ** 31
    g = torch.Generator().manual_seed(64)
    w = torch.randn(48, 48, 3, 3, generator=g) / np.sqrt(9 * 48)
    b = (torch.randn(48, generator=g) * 0.1).to(dev)
    packed, unscale = pack_conv3x3_w96(w.numpy(), 48)
    wp = torch.from_numpy(packed.view(np.int16)).to(dev)
    y = hip_ctx.conv3x3_f16x3_s8(x, wp, b, 48, unscale, relu=True)
    for pair in ((0, 31), (32, 63)):
        small = hip_ctx.conv3x3_f16x3_s8(x[list(pair)].contiguous(), wp, b, 48, unscale, relu=True)
        for j, i in enumerate(pair):
            assert torch.equal(y[i], small[j]), i
    del x, y, small
    torch.cuda.empty_cache()
