"""Kernel parity at the edges for the cut-point refinement entry points of ac_guard.hip (moving mean square in dB, next-quiet scan,
window argmin, nearest zero crossing, slow quiet guard, pause cut points) and the two host layers that turn their answers into
sample indices (`PureVocalPauseDetector._calculate_precise_cut_points`, `cutting.refine.finalize_cut_points`).  Each check compares
with a plain numpy / float64 statement of the same operation (oracle/refine.py, oracle/detector.py, or one written here) at the
shapes where these kernels go wrong: block and tile edges, multi-block carries, clipped windows, track ends, ties, NaN, denormals.
Every check states its tolerance and why.  GPU box only."""
import contextlib

import numpy as np
import pytest
import torch

from audio_cut_amd import config as AC
from audio_cut_amd.cutting import refine as R
from audio_cut_amd.detectors.pure_vocal_pause_detector import PureVocalPause, PureVocalPauseDetector
from audio_cut_amd.testing import signals
from oracle import config as OCfg, detector as OD, refine as OR

pytestmark = pytest.mark.gpu
SR = 44100
ZERO_DB = 20.0 * np.log10(np.sqrt(0.0 + 1e-12) + 1e-12)       # the dB value of a window of exact zeros


# ---------------------------------------------------------------------------------------------------------------------
# moving_meansq_db
# ---------------------------------------------------------------------------------------------------------------------
def _meansq_db_kernel_statement(x, win):
    """The kernel's definition for every n: output i is the mean of x^2 over [i - win//2, i - win//2 + win) clipped to [0, n),
    divided by win.  For n >= win this is np.convolve(sq, ones / win, 'same'); zero padding on both sides keeps that
    alignment for n < win too, where np.convolve itself would swap its operands."""
    sq = np.square(x.astype(np.float64))
    ms = np.convolve(np.pad(sq, (win, win)), np.ones(win) / float(win), mode="same")[win:win + len(x)]
    return 20.0 * np.log10(np.sqrt(ms + 1e-12) + 1e-12)


def _meansq_signals(n, seed):
    rng = np.random.default_rng(seed)
    gated = (0.5 * rng.standard_normal(n)).astype(np.float32)
    runs = rng.integers(0, n, 6)
    for r, ln in zip(runs, rng.integers(1, max(2, n // 3), 6)):
        gated[r:r + ln] = 0.0                                      # exact-zero runs of every length, some touching n
    gated[: max(1, n // 7)] = 0.0                                  # and one touching 0
    tiny = (1e-6 * rng.standard_normal(n)).astype(np.float32)
    full = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    return {"gated": gated, "tiny": tiny, "full": full}


@pytest.mark.parametrize("win", [1, 2, 255, 256, 257, 441, 3528, 8191, 8192])
def test_moving_meansq_db_edges(hip_ctx, win):
    """`ac_moving_meansq_db_f64` at windows on the edges of the per-thread chunk (255/256/257: one or two elements per thread),
    the 64 KiB dynamic-LDS limit (8192 needs 128 KiB through hipFuncSetAttribute and fills MS_PT) and win 1 / 2, over
    n = 1, win - 1, win, win + 1, 3 win, 3 win + 1 (partial last block) and 2 s, on a signal with exact-zero runs, one at
    1e-6 and one at full scale.  atol 1e-9 dB (the float64 sums differ from np.convolve's only in order); windows of exact
    zeros are bit-equal and sit exactly where the reference has them (np.argmin ties resolve on them).  For n < win the kernel
    keeps its own centring (n outputs; the host builds the reference's lookup itself, see test_prepare_lookup_short_wave)."""
    rng = np.random.default_rng(win)
    ns = sorted({1, win - 1, win, win + 1, 3 * win, 3 * win + 1} - {0})
    for name, sig in _meansq_signals(3 * win + 1, win).items():
        for n in ns:
            x = np.ascontiguousarray(sig[:n])
            got = hip_ctx.moving_meansq_db(hip_ctx.to_device(x), win).cpu().numpy()
            ref = OR.moving_meansq_db(x, win) if n >= win else _meansq_db_kernel_statement(x, win)
            assert got.shape == (n,), (name, n)
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9, err_msg=f"{name} n={n}")
            assert np.array_equal(got == ZERO_DB, ref == ZERO_DB), (name, n)
    # a few seconds of all three levels in one wave (block carries across many workgroups)
    n = 2 * SR
    parts = _meansq_signals(n // 3 + 1, win + 1)
    x = np.concatenate([parts["gated"], parts["tiny"], parts["full"]])[:n]
    x[rng.integers(0, n - 20000):][:20000] = 0.0
    got = hip_ctx.moving_meansq_db(hip_ctx.to_device(x), win).cpu().numpy()
    ref = OR.moving_meansq_db(x, win)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)
    silent = ref == ZERO_DB
    assert silent.any() and np.array_equal(got == ZERO_DB, silent)


@pytest.mark.parametrize("n", [1, 5, 300, 440, 441, 442, 3000])
def test_prepare_lookup_short_wave(hip_ctx, n):
    """`_Wave.prepare_lookup` against the reference's `_prepare_quiet_lookup` (OR.prepare_quiet_lookup) at the live 10 ms guard
    window (441 samples).  For a wave shorter than the window np.convolve swaps its operands and returns `win` values with another
    centring; the kernel returns n values of its own window, so the host builds that lookup with numpy.  rms_db atol 1e-9 dB
    (summation order) and the same length; next_quiet exact."""
    rng = np.random.default_rng(n)
    x = (0.01 * rng.standard_normal(n)).astype(np.float32)
    x[n // 3: n // 2] = 0.0
    w = R._Wave(hip_ctx, hip_ctx.to_device(x), n, SR)
    lk = w.prepare_lookup(10.0, -60.0)
    ref = OR.prepare_quiet_lookup(x, SR, 10.0, -60.0)
    got = lk.rms_db.cpu().numpy()
    assert got.shape == ref.rms_db.shape
    np.testing.assert_allclose(got, ref.rms_db, rtol=0, atol=1e-9)
    assert np.array_equal(lk.next_quiet.cpu().numpy(), ref.next_quiet)
    if n < 441:            # finding 3: the kernel's own series is not the reference's lookup here
        own = hip_ctx.moving_meansq_db(hip_ctx.to_device(x), 441).cpu().numpy()
        assert own.shape != ref.rms_db.shape


# ---------------------------------------------------------------------------------------------------------------------
# next_leq_scan
# ---------------------------------------------------------------------------------------------------------------------
NQ_BLK = 4096


def _nq_patterns(n, rng):
    out = {"none": np.ones(n), "all": np.zeros(n)}               # "all": every element EQUAL to the floor (<=, not <)
    last = np.ones(n); last[-1] = -1.0
    out["last"] = last
    edges = np.ones(n)
    blk = np.arange(0, n, NQ_BLK)
    pick = blk[rng.random(len(blk)) < 0.15]                       # block edges of some blocks: 4095 of one, 0 of the next
    edges[np.clip(pick - 1, 0, n - 1)] = -1.0
    edges[pick[::2]] = -1.0
    if n > 2 * NQ_BLK:
        edges[: n // 2] = 1.0                                     # the first half of the blocks have none: long carries
    out["edges"] = edges
    sparse = np.ones(n)
    nb = (n + NQ_BLK - 1) // NQ_BLK
    hit_blocks = np.flatnonzero(rng.random(nb) < 0.05)
    pos = hit_blocks * NQ_BLK + rng.integers(0, NQ_BLK, len(hit_blocks))
    sparse[pos[pos < n]] = -2.5
    out["sparse"] = sparse
    return out


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 256 * 4096, 256 * 4096 + 1, 300 * 4096 + 17, 10_584_000])
def test_next_leq_scan_edges(hip_ctx, n):
    """`ac_next_leq_scan` on synthetic float64 series: one block, one block +- 1, exactly 256 blocks (each carry thread owns one
    block), 257 and 301 blocks (threads own two: the per-thread carry loop) and a 4-minute track (2584 blocks, 11 per thread).
    Hits at block edges (4095 / 4096), only at the last element, nowhere (all -1), everywhere (equal to the floor) and sparse.
    Integer output: exact against OR.next_leq_scan."""
    rng = np.random.default_rng(n)
    for name, db in _nq_patterns(n, rng).items():
        got = hip_ctx.next_leq_scan(hip_ctx.to_device(db), 0.0).cpu().numpy()
        assert np.array_equal(got, OR.next_leq_scan(db, 0.0)), (n, name)


# ---------------------------------------------------------------------------------------------------------------------
# window_argmin
# ---------------------------------------------------------------------------------------------------------------------
def test_window_argmin_edges(hip_ctx):
    """`ac_window_argmin_f64` over a series made of runs of equal values (coarse levels and long runs of the exact-zero dB value):
    every window has many equal minima across threads and waves, so the first index must win.  Windows of len 1, 255, 256, 257,
    19845, start = 0, start = n - 1, start + len past n (clipped to n).  Every start is in [0, n), as the host guarantees.
    arg, db[start] and db[arg] exact (pure selection)."""
    rng = np.random.default_rng(11)
    n = 50_000
    db = np.round(rng.uniform(-80.0, -20.0, n), 0)                # integer dB levels: ties everywhere
    db = np.repeat(db[: n // 8], 8)[:n]
    for r in rng.integers(0, n - 3000, 6):
        db[r:r + int(rng.integers(300, 3000))] = ZERO_DB
    starts, lens = [], []
    for ln in (1, 2, 255, 256, 257, 600, 19845):
        for s in (0, 1, 255, 256, n - 1, n - ln, n - ln // 2 - 1, *rng.integers(0, n, 6)):
            if 0 <= s < n:
                starts.append(int(s)); lens.append(int(ln))
    starts += [n - 1, n - 10, 0]; lens += [19845, 19845, n + 5]
    s = np.array(starts, dtype=np.int64); ln = np.array(lens, dtype=np.int64)
    arg, val = hip_ctx.window_argmin(hip_ctx.to_device(db), s, ln)
    for q in range(len(s)):
        e = min(n, s[q] + ln[q])
        k = s[q] + int(np.argmin(db[s[q]:e]))
        assert arg[q] == k, (q, s[q], ln[q], arg[q], k)
        assert val[q, 0] == db[s[q]] and val[q, 1] == db[k]


# ---------------------------------------------------------------------------------------------------------------------
# zero_cross_nearest
# ---------------------------------------------------------------------------------------------------------------------
def _zero_cross_track():
    """Positive background (no crossing anywhere) with planted features at centres 2000 apart; a noisy stretch at the end; exact
    zeros at samples 0 and n - 1."""
    rng = np.random.default_rng(21)
    n = 120_000
    x = (0.25 + 0.5 * rng.random(n)).astype(np.float32)
    centres = []
    c = 3000

    def nxt():
        nonlocal c
        c += 2000
        centres.append(c)
        return c

    for d in (0, 1, 2, 31, 63, 64, 65, 200, 352):
        k = nxt(); x[k - d: k + d + 1] = -0.5; x[k - d - 1] = 0.5; x[k + d + 1] = 0.5   # crossings at k - d - .5, k + d + .5: a tie
    for d in (1, 3, 40, 300):
        k = nxt(); x[k - d] = 0.0; x[k + d] = 0.0                                        # exact zeros equally far on both sides
        k = nxt(); x[k - d] = 0.0                                                        # a zero on the left only (at l, then at r)
        k = nxt(); x[k + d] = 0.0; x[k + d + 1] = 0.0                                    # zeros at l and r of one pair
    for d in (0, 1, 50):
        k = nxt(); x[k + d] = 1e-20; x[k + d + 1] = -1e-20; x[k + d + 2] = -1e-20       # product -1e-40 (float32 denormal) at
        #                                                                                  k + d + .5; the next crossing is near k + d + 2
        k = nxt(); x[k + d] = -0.3; x[k - d] = -0.3                                      # fractional crossings on both sides
    for _ in range(8):
        k = nxt(); m = int(rng.integers(3, 400)); x[k - m: k + m] *= np.where(rng.random(2 * m) < 0.5, -1, 1).astype(np.float32)
    x[-20_000:] = rng.standard_normal(20_000).astype(np.float32)
    x[-20_000:][rng.random(20_000) < 0.01] = 0.0
    x[0] = 0.0
    x[-1] = 0.0
    return x, centres


@pytest.mark.parametrize("half", [1, 2, 63, 64, 65, 353])
def test_zero_cross_nearest_edges(hip_ctx, half):
    """`ac_zero_cross_nearest` at half-widths around the wave size (63 / 64 / 65 pairs per lane), queries at 1, half, n - 1 - half
    and n - 1 (the search clipped to [1, n - 1]), exact zeros at l, at r and at both, crossings equally far on both sides (the
    first wins), a crossing between samples of 1e-20 (float32 product of denormal size) and a noisy stretch with random queries.
    Bit-equal to OR.zero_cross_snap(..., legacy_promotion=True) for every query: the position arithmetic is the reference's
    float32 then float64, a pure selection otherwise."""
    x, centres = _zero_cross_track()
    n = len(x)
    rng = np.random.default_rng(half)
    idx = [1, 2, half, half + 1, n - 1 - half, n - 2, n - 1]
    for c in centres:
        idx += [c, c - 1, c + 1]
    idx += list(rng.integers(n - 20_000, n - 1, 300))
    idx = np.array([i for i in idx if 1 <= i <= n - 1], dtype=np.int64)
    pos = hip_ctx.zero_cross_nearest(hip_ctx.to_device(x), idx, half)
    win_ms = half * 1000.0 / SR
    assert max(1, int(round(win_ms / 1000.0 * SR))) == half
    for q, i in enumerate(idx):
        t = int(i) / SR
        assert int(round(t * SR)) == i
        ref = OR.zero_cross_snap(x, SR, t, win_ms, legacy_promotion=True)
        got = t if np.isnan(pos[q]) else float(pos[q]) / SR
        assert got == ref, (half, q, int(i), pos[q], ref * SR)


# ---------------------------------------------------------------------------------------------------------------------
# quiet_guard_slow
# ---------------------------------------------------------------------------------------------------------------------
def _slow_guard_statement(x, c, span, win):
    """The kernel's operation (refine.py:113-157 up to the decision): -1 / NaN when end <= c + 1; for seg <= win the level is the
    raw signed sample, so a negative one gives NaN; np.argmin returns the first NaN, else the first minimum."""
    n = len(x)
    c = max(0, c)
    end = min(n, c + span)
    if end <= c + 1:
        return -1, np.nan, np.nan
    seg = x[c:end]
    if seg.size <= win:
        with np.errstate(invalid="ignore"):
            db = 20.0 * np.log10(seg.astype(np.float64) + 1e-12)
    else:
        padded = np.pad(seg, (0, win - 1), mode="edge")
        lvl = np.sqrt(np.convolve(padded * padded, np.ones(win) / float(win), mode="valid") + 1e-12)
        db = 20.0 * np.log10(lvl + 1e-12)
    k = int(np.argmin(db))
    return k, db[0], db[k]


@pytest.mark.parametrize("span,win", [(6615, 441), (19845, 3528), (32768, 3528), (300, 7), (6615, 7)])
def test_quiet_guard_slow_edges(hip_ctx, span, win):
    """`ac_quiet_guard_slow`, both branches: windows over random noise with exact-zero runs (no ties but exact ones: exact arg)
    at the live 150 ms / 10 ms, the detector's span, and the 32768-sample limit (128 windows per thread, 145 KiB of LDS); and the
    raw-sample branch (seg <= win, queries within win of n) over signed samples with exact zeros and over a non-negative tail.
    Queries with end <= c + 1 return -1.  Regression: with a window shorter than a thread's run of windows (7 at a 6615 span: 26
    per thread) the windows share no core, and the head / core / tail sums counted samples twice.  arg exact (np.argmin's first NaN included); values atol 1e-9 dB, NaN where the statement
    has NaN (the float64 sums differ from np.convolve's in order only)."""
    rng = np.random.default_rng(span + win)
    n = 6 * span + 3 * win
    x = (0.05 * rng.standard_normal(n)).astype(np.float32)
    x[2 * span: 2 * span + span // 2] = 0.0
    x[4 * span + 17: 4 * span + 17 + win + 5] = 0.0
    tail = n - win - 40
    x[tail: tail + 8] = 0.0
    x[n - win // 3:] = np.abs(x[n - win // 3:])                    # a non-negative tail: no NaN, ties among its exact zeros
    x[n - win // 3 + 3: n - win // 3 + 9] = 0.0
    x[n - 5] = 0.0
    idx = [0, 1, -3, 255, 2 * span - win, 2 * span + 5, 4 * span, *rng.integers(0, n - span, 12)]
    idx += [n - span, n - span - 1, n - win - 1, n - win, n - win + 1, tail, tail + 3, n - win // 3, n - win // 3 + 2, n - 6, n - 3,
            n - 2, n - 1]
    idx += list(rng.integers(n - win, n - 1, 20))
    idx = np.array(idx, dtype=np.int64)
    arg, val = hip_ctx.quiet_guard_slow(hip_ctx.to_device(x), idx, span, win)
    raw_nan = 0
    for q, c in enumerate(idx):
        k, d0, dk = _slow_guard_statement(x, int(c), span, win)
        assert arg[q] == k, (q, int(c), arg[q], k)
        if k < 0:
            continue
        np.testing.assert_allclose(val[q], [d0, dk], rtol=0, atol=1e-9, equal_nan=True, err_msg=f"q={q} c={int(c)}")
        raw_nan += int(np.isnan(dk))
    assert raw_nan > 0                                             # the first-NaN rule was exercised


# ---------------------------------------------------------------------------------------------------------------------
# pause_cut_points
# ---------------------------------------------------------------------------------------------------------------------
def _pause_statement(x, a, b, win, guard):
    """pure_vocal_pause_detector.py:1047-1078 with OD._local_rms; a cut at or past n has no look-ahead and no sample."""
    n = len(x)
    m = b - a
    if m <= 1:
        return -1, 0, 0
    seg = x[a:b]
    c = a + int(np.argmin(OD._local_rms(seg, win)))
    if guard > 0:
        g_end = min(n, c + guard)
        if g_end > c:
            c = min(g_end - 1, c + int(np.argmin(OD._local_rms(x[c:g_end], win))))
    return c, int(np.sum(seg == 0)), int(c < n and x[c] != 0)


def _noise(rng, n, amp):
    return (amp * rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _halves(x, a, m, rng, quiet_second=True):
    h = m // 2
    loud, quiet = _noise(rng, h, 0.1), _noise(rng, m - h, 0.001)
    x[a:a + m] = np.concatenate([loud, quiet]) if quiet_second else np.concatenate([_noise(rng, h, 0.001), _noise(rng, m - h, 0.1)])


def _zero_run_at_output(x, a, i0, win, length):
    """Exact zeros such that the first output of a pause starting at a whose window lies inside them is i0 (m >= win)."""
    z0 = a + i0 + (win - 1) // 2 - win + 1                           # output i sums samples [i + off - win + 1, i + off]
    x[z0:z0 + length] = 0.0


def _pause_cases(win):
    """(x, a, b) groups.  Minima are exact-zero windows or clearly separated halves, so float32 envelopes summed in another order
    cannot reorder them."""
    rng = np.random.default_rng(win)
    cases = []
    # main track: a 6 s pause with its minimum in workgroup 0's SECOND tile, minima on a 4096-output tile edge, equal minima in
    # two workgroups, a pause at a = 0, short pauses (2, win - 1, win, win + 1) with either half quieter
    n = 12 * SR
    x = _noise(rng, n, 0.1)
    pa, pb = [], []

    def add(a, m):
        pa.append(a); pb.append(a + m)

    add(10_000, 6 * SR); _zero_run_at_output(x, 10_000, 64 * 4096 + 1000, win, 3 * win)
    add(280_000, 20_000); _zero_run_at_output(x, 280_000, 4096, win, 3 * win)
    add(302_000, 20_000); _zero_run_at_output(x, 302_000, 4095, win, 3 * win)
    add(324_000, 30_000); _zero_run_at_output(x, 324_000, 3000, win, 3 * win); _zero_run_at_output(x, 324_000, 9000, win, 3 * win)
    add(0, 6000); _zero_run_at_output(x, 0, 2000, win, 2 * win)
    a = 360_000
    for m in (2, win - 1, win, win + 1):
        for quiet_second in (True, False):
            if m >= 2:
                _halves(x, a, m, rng, quiet_second)
            add(a, m)
            a += max(3 * win, 3000) + 5292
    add(a, 1)                                                       # m <= 1: cut -1
    cases.append((x, np.array(pa), np.array(pb)))
    # pauses that end at n: a short one whose first cut lands past n (finding 1), one whose cut lands exactly on n, a long one
    for m in (max(2, win // 2), max(2, win - 1)):
        n = 30_000
        x = _noise(rng, n, 0.1)
        _halves(x, n - m, m, rng, True)
        cases.append((x, np.array([n - m, n - 20_000]), np.array([n, n])))
        _zero_run_at_output(x, n - 20_000, 9000, win, 2 * win)
    # the look-ahead runs into n with fewer than win samples left: its 'same' output is then win long, the cut clamps to n - 1
    for quiet_second in (True, False):
        n = 30_000
        x = _noise(rng, n, 0.1)
        m = 800 if win > 800 else 2
        a = n - win - 200
        _halves(x, a, m, rng, True)
        _halves(x, n - 201, 201, rng, quiet_second)
        cases.append((x, np.array([a]), np.array([a + m])))
    # the look-ahead's minimum on its last output (its window is exact zeros): catches an off-by-one in the look-ahead length
    n = 40_000
    x = _noise(rng, n, 0.1)
    m = 800 if win > 800 else 2
    a = 10_000
    _halves(x, a, m, rng, True)
    cut = a + win - 1 if win > 800 else a
    x[cut + 5292 - 552: cut + 5292] = 0.0
    cases.append((x, np.array([a]), np.array([a + m])))
    return cases


@pytest.mark.parametrize("win,guard", [(1102, 5292), (2, 5292), (7, 64), (1102, 0)])
def test_pause_cut_points_edges(hip_ctx, win, guard):
    """`ac_pause_cut_points` at the live 25 ms / 120 ms (1102 / 5292), at win 2 and 7 and without look-ahead.  A 6 s pause whose
    minimum lies in a later tile of a workgroup (past 64 x 4096 outputs), minima on a tile edge (4095 / 4096), equal minima in two
    workgroups (the first wins through the packed atomicMin), a pause at a = 0, pauses of 2, win - 1, win and win + 1 samples,
    pauses that end at n (the first cut lands at or past n when the pause is shorter than win: finding 1), look-aheads clipped by
    n with fewer than win samples left (the 'same' output is then win long: clamp to g_end - 1), a look-ahead minimum on its last
    output.  cut and both aux columns exact against the OD._local_rms statement (integer decisions on exact-zero windows or
    clearly separated envelopes).  Regression: a window shorter than a thread's run of 16 outputs (win 2 to 14) shares no core
    with its neighbours, and the run's head / core / tail sums counted samples twice."""
    past_end = 0
    for x, a, b in _pause_cases(win):
        cut, aux = hip_ctx.pause_cut_points(hip_ctx.to_device(x), a, b, win, guard)
        for q in range(len(a)):
            c, zeros, nz = _pause_statement(x, int(a[q]), int(b[q]), win, guard)
            assert cut[q] == c, (win, guard, int(a[q]), int(b[q]), cut[q], c)
            assert aux[q, 0] == zeros and aux[q, 1] == nz, (q, aux[q], zeros, nz)
            past_end += int(c >= len(x))
    if win > 2:
        assert past_end > 0                                          # finding 1 was reached


# ---------------------------------------------------------------------------------------------------------------------
# host decision layers
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _overrides(d):
    saved_p, saved_o = AC.snapshot(), {k: OCfg.get_config(k) for k in d}
    AC.set_runtime_config(d)
    OCfg.set_runtime_config(d)
    try:
        yield
    finally:
        AC.restore(saved_p)
        OCfg.set_runtime_config(saved_o)


def _floor_pauses(pct, rng):
    """Short pauses whose count of exact zeros sits at, just below and just above the order statistics np.percentile
    interpolates (lo_i, lo_i + 1), one 1500-sample pause with a constant quiet stretch (an exact tie the first window wins), and
    pauses that end at n whose first cut lands at or past n, with a zero and with a positive floor."""
    n = 40 * SR
    x = _noise(rng, n, 0.1)
    spans = []
    a = 2000
    for m in (2, 3, 5, 20, 21, 41, 101, 400):
        lo_i = int(np.floor((pct / 100.0) * (m - 1)))
        for z in sorted({max(0, lo_i - 1), lo_i, lo_i + 1, min(m, lo_i + 2)}):
            seg = _noise(rng, m, 0.05)
            seg[rng.choice(m, z, replace=False)] = 0.0
            x[a:a + m] = seg
            spans.append((a, a + m))
            a += 8000
    x[a:a + 200] = _noise(rng, 200, 0.5); x[a + 200:a + 1400] = 1e-3; x[a + 1400:a + 1500] = _noise(rng, 100, 0.5)
    spans.append((a, a + 1500))
    # the end: a pause of 551 samples, quieter second half, ending at n (first cut at n + 550)
    m = 551
    _halves(x, n - m, m, rng, True)
    spans.append((n - m, n))
    return x, spans


@pytest.mark.parametrize("pct,allow", [(5.0, 0.0), (37.0, 0.0), (5.0, 1.5)])
def test_precise_cut_points_host_against_oracle(hip_ctx, pct, allow):
    """`_calculate_precise_cut_points` (kernel cut + the host's zero-count form of `np.percentile(|seg|, pct) > 0`) against
    OD.precise_cut_points: cut_point and quality_grade equal.  The pause that ends at n has its first cut past the end; the
    reference keeps that cut when the floor is zero and raises IndexError at vocal[cut] otherwise, where this build falls back to
    the pause midpoint (grade B), as documented in the detector.  Both are checked, with a zero floor (its samples zeroed) and a
    positive one."""
    rng = np.random.default_rng(int(pct * 10 + allow * 100))
    x, spans = _floor_pauses(pct, rng)
    n = len(x)
    det = PureVocalPauseDetector(SR, ctx=hip_ctx)
    raised = 0
    for zero_end in (False, True):
        if zero_end:
            x = x.copy(); x[n - 551:] = 0.0; x[n - 551] = 0.05       # the floor of the end pause is zero
        xd = hip_ctx.to_device(x)
        with _overrides({"vocal_pause_splitting.silence_floor_percentile": pct, "vocal_pause_splitting.silence_floor_allowance": allow}):
            mk = lambda: [PureVocalPause(a / SR, b / SR, (b - a) / SR, "test", 1.0, {}) for a, b in spans]
            got = det._calculate_precise_cut_points(mk(), xd)
            for g, p in zip(got, mk()):
                a, b = int(round(p.start_time * SR)), int(round(p.end_time * SR))
                try:
                    (r,) = OD.precise_cut_points([OD.Pause(p.start_time, p.end_time, p.duration, "test", 1.0)], x, SR)
                except IndexError:
                    raised += 1
                    assert b == n and (g.cut_point, g.quality_grade) == ((a + (b - a) // 2) / SR, "B"), (a, b, g.cut_point)
                    continue
                assert (g.cut_point, g.quality_grade) == (r.cut_point, r.quality_grade), (a, b, g.cut_point * SR, r.cut_point * SR)
                if b == n:
                    assert r.cut_point * SR >= n                   # the reference's own cut past the end, kept
    assert raised == 1                                               # positive floor: the reference raises, once


def _refine_tracks():
    rng = np.random.default_rng(5)
    mix = signals.c1_sine_silence(2.0, seed=5)
    voc = signals.vocal_like(2.0, seed=5)
    for w in (mix, voc):
        w[-int(0.3 * SR):] = (0.1 * rng.standard_normal(int(0.3 * SR))).astype(np.float32)   # signed, loud tail: the raw branch
    return mix, voc


@pytest.mark.parametrize("min_boundary_s", [0.5, 0.0])
def test_finalize_cut_points_against_oracle(hip_ctx, min_boundary_s):
    """`cutting.refine.finalize_cut_points` against OR.finalize_cut_points on 20 random cut lists with points near 0, near n and
    within the 150 ms search span of the end (the slow guard's raw-sample branch within 10 ms of it), at the default
    min_boundary_s and at 0 (points near the end survive: the first-NaN rule shows), plus a wave shorter than the guard window
    (the reference's lookup of `win` values).  sample_boundaries exact; every adjustment's times and score equal."""
    mix, voc = _refine_tracks()
    rng = np.random.default_rng(int(min_boundary_s * 10) + 1)
    dur = len(mix) / SR
    short = (0.01 * rng.standard_normal(300)).astype(np.float32)
    short[100:180] = 0.0
    jobs = []
    for j in range(20):
        k = int(rng.integers(2, 8))
        ts = list(rng.uniform(0.0, dur, k))
        ts += [float(rng.uniform(0.0, 0.02)), float(dur - rng.uniform(0.0, 0.15)), float(dur - rng.uniform(0.0, 0.01)), 1.0 / SR,
               (len(mix) - 1) / SR, dur]
        jobs.append((mix, voc, ts))
    for _ in range(4):
        jobs.append((short, short[::-1].copy(), list(rng.uniform(0.0, 300 / SR, 3))))
    for mw, vw, ts in jobs:
        scores = list(rng.uniform(0.1, 1.0, len(ts)))
        ctx = R.CutContext(sr=SR, mix_wave=mw, vocal_wave=vw, hip=hip_ctx)
        got = R.finalize_cut_points(ctx, [R.CutPoint(t, s) for t, s in zip(ts, scores)], min_boundary_s=min_boundary_s)
        ref = OR.finalize_cut_points(SR, mw, vw, [OR.Cut(t, s) for t, s in zip(ts, scores)], min_boundary_s=min_boundary_s)
        assert got.sample_boundaries == ref.sample_boundaries, (ts, got.sample_boundaries, ref.sample_boundaries)
        assert [p.t for p in got.final_points] == ref.times
        assert [(a.raw_time, a.guard_time, a.final_time, a.score) for a in got.adjustments] == \
            [(a.raw_time, a.guard_time, a.final_time, a.score) for a in ref.adjustments], ts
