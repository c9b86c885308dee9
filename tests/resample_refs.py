"""Plain float64 reference of the polyphase resamplers (audio_cut_amd/csrc/ac_common.h `ac_polyphase_dot_wave`, shared by
ac_resample_poly, ac_resample_poly_segments and ac_resample_poly_pcm16), written from the header's definition with the SAME taps the
kernel is given, so that no filter-design difference has to be absorbed by a tolerance: the kernel's float64 sum over exact products
of float32 operands is pinned to half a float32 ulp.  numpy only; tests/test_resample_refs_host.py pins this module against
scipy.signal.resample_poly on the CPU and checks that it rejects three restated mutants, tests/test_resample_pcm_edges_gpu.py then
holds the kernels to it."""
import math

import numpy as np

MUTANTS = ("t_hi_drops_last_tap", "t_lo_one_too_high", "n_pre_remove_plus_one")


def n_out_of(n, up, down):
    """ceil(n up / down): scipy.signal.resample_poly's output length."""
    return -(-n * up // down)


def padded_taps(hfull, up):
    """(hfull zero-padded to a multiple of `up` as float32, taps per row)."""
    hfull = np.asarray(hfull)
    assert hfull.dtype == np.float32 and hfull.ndim == 1
    tpp = -(-hfull.size // up)
    hpad = np.zeros(tpp * up, dtype=np.float32)
    hpad[:hfull.size] = hfull
    return hpad, tpp


def tap_range(m, n, up, down, tpp, n_pre_remove, mutant=None):
    """(j0, p, t_lo, t_hi) of output m: x[j0 - t] meets rows[p][t] for t_lo <= t <= t_hi (empty when t_lo > t_hi).
    `mutant` restates one of three off-by-one errors (MUTANTS) for the self-check of the host test."""
    if mutant == "n_pre_remove_plus_one":
        n_pre_remove += 1
    i = (m + n_pre_remove) * down
    j0 = i // up
    p = i - j0 * up
    t_lo = max(0, j0 - (n - 1))
    t_hi = min(j0, tpp - 1)
    if mutant == "t_hi_drops_last_tap":
        t_hi = min(j0, tpp - 2)
    if mutant == "t_lo_one_too_high" and j0 - (n - 1) > 0:
        t_lo += 1
    return j0, p, t_lo, t_hi


def polyphase_ref64(x, up, down, hfull, n_pre_remove, n_out, mutant=None, outputs=None):
    """y[m] = sum_{t = t_lo}^{t_hi} rows[p][t] x[j0 - t] with i = (m + n_pre_remove) down, j0 = i // up, p = i - j0 up,
    t_lo = max(0, j0 - (n - 1)), t_hi = min(j0, tpp - 1) and rows[p][t] = hfull[p + t up] (float32, zero-padded rows).
    Every product is formed in float64 (exact for float32 operands) and a row is summed with math.fsum, i.e. y is the correctly
    rounded sum of the terms.  Returns (y [n_out] float64, mag [n_out] float64 = sum of |term|).  An empty tap range gives +0.0;
    non-finite terms propagate as IEEE addition dictates (a zero-padded tap times NaN is NaN).  `outputs`: evaluate only these m
    (the others stay 0.0), for spot checks of long signals."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x64.size
    hpad, tpp = padded_taps(hfull, up)
    rows = hpad.astype(np.float64).reshape(tpp, up).T          # rows[p][t] = hpad[p + t * up]
    y = np.zeros(n_out, dtype=np.float64)
    mag = np.zeros(n_out, dtype=np.float64)
    for m in (range(n_out) if outputs is None else outputs):
        j0, p, t_lo, t_hi = tap_range(m, n, up, down, tpp, n_pre_remove, mutant)
        if t_lo > t_hi:
            continue
        t = np.arange(t_lo, t_hi + 1)
        with np.errstate(invalid="ignore"):
            terms = rows[p, t] * x64[j0 - t]
        if np.all(np.isfinite(terms)):
            y[m] = math.fsum(terms)
            mag[m] = math.fsum(np.abs(terms))
        else:                                                   # NaN / Inf: only the class of the result matters
            with np.errstate(invalid="ignore"):
                y[m] = np.sum(terms)
                mag[m] = np.sum(np.abs(terms))
    return y, mag


def ulp32(y64):
    """Spacing of float32 in the binade of |y64| (float64 in, float64 out), with the denormal floor 2^-149."""
    a = np.abs(np.asarray(y64, dtype=np.float64))
    _, e = np.frexp(a)                                          # a = f 2^e, 0.5 <= f < 1: the binade is [2^(e-1), 2^e)
    return np.maximum(np.where(a > 0, np.ldexp(1.0, e.astype(np.int64) - 24), 0.0), 2.0 ** -149)      # frexp(0) = (0, 0)


def assert_same_taps(got_f32, y64, mag, tpp, label="", quiet=False):
    """|got - y64| <= ulp32(y64) / 2 + tpp 2^-52 mag, sample by sample.  The first term is the final rounding of a float64 sum to
    float32; the second bounds the error of a float64 sum of at most tpp terms in ANY order (each of the at most tpp - 1 additions,
    fused with its product or not, errs by at most 2^-53 of a partial sum that never exceeds mag (1 + tpp 2^-53): below
    tpp 2^-52 mag with room to spare).  When a sum that close to a binade's upper end rounds up into the next one, it rounds to the
    power of two itself, which lies within the second term.  Non-finite samples must agree in class (NaN with NaN, an infinity
    with the same infinity).  Prints the worst error-to-bound ratio and how many samples differ from float32(y64) at all (unless
    `quiet`); returns both."""
    got = np.asarray(got_f32)
    assert got.dtype == np.float32 and got.shape == y64.shape == mag.shape, (got.dtype, got.shape, y64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(y64)), f"{label}: NaN set differs, first at {_first(np.isnan(got) != np.isnan(y64))}"
    inf = np.isinf(y64)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf].astype(np.float64), y64[inf]), f"{label}: infinities differ"
    fin = np.isfinite(y64)
    err = np.abs(got[fin].astype(np.float64) - y64[fin])
    bound = 0.5 * ulp32(y64[fin]) + tpp * 2.0 ** -52 * mag[fin]
    with np.errstate(over="ignore"):
        rounded = y64[fin].astype(np.float32)
    differ = int(np.count_nonzero(got[fin] != rounded))
    ratio = err / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    if not quiet:                                               # a caller that loops over many cases prints their maximum instead
        print(f"{label}: worst error / bound {worst:.3f}, {differ} of {got.size} differ from float32(y64)")
    if worst > 1.0:
        k = int(np.flatnonzero(fin)[int(np.argmax(ratio > 1.0))])
        raise AssertionError(f"{label}: output {k}: got {got[k]!r}, reference {y64[k]!r}, error {abs(float(got[k]) - y64[k]):.3e} "
                             f"> bound {0.5 * float(ulp32(y64[k])) + tpp * 2.0 ** -52 * mag[k]:.3e}; worst ratio {worst:.3f}")
    return worst, differ


def _first(mask):
    return int(np.argmax(mask))


def impulse_train(up, down, hfull, n_pre_remove):
    """Sparse input on which every output is ONE tap: unit impulses at q_k = k s, 1 <= k <= down, s the smallest spacing >= tpp + 1
    that is coprime with `down`, followed by tpp zeros.  An impulse at q answers at the outputs with i = (m + n_pre_remove) down in
    [q up, (q + tpp) up) with the tap hpad[i - q up]; the responses do not overlap (s > tpp), so every product but one is a tap
    times 0.0 and the output is float32(tap) exactly, in any summation order.  gcd(s up, down) = 1 makes the `down` impulses start
    in `down` different residues of i modulo `down`: together they read every index of [0, tpp up) exactly once.  (k starts at 1,
    not 0: the outputs that would read the first half of an impulse at sample 0 lie in front of output 0.)
    Returns (x float32 [n], expected float32 [n_out], idx int64 [n_out]: the index of hpad behind each output, -1 where none)."""
    hpad, tpp = padded_taps(hfull, up)
    s = tpp + 1
    while math.gcd(s, down) != 1:
        s += 1
    q = s * np.arange(1, down + 1, dtype=np.int64)
    n = int(q[-1]) + tpp
    x = np.zeros(n, dtype=np.float32)
    x[q] = 1.0
    n_out = n_out_of(n, up, down)
    i = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down
    j0 = i // up
    k = np.searchsorted(q, j0, side="right") - 1                # the last impulse at or in front of j0
    idx = np.where(k >= 0, i - q[np.maximum(k, 0)] * up, -1)
    idx = np.where((idx >= 0) & (idx < tpp * up), idx, -1)
    expected = np.where(idx >= 0, hpad[np.maximum(idx, 0)], np.float32(0.0)).astype(np.float32)
    return x, expected, idx
