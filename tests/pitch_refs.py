"""References and input builders for the pitch kernels (audio_cut_amd/csrc/ac_pitch.hip): k_pyin_viterbi, k_pyin_observe and
k_lpc_formants, stage by stage.  numpy / scipy only; tests/test_pitch_kernels_gpu.py pins this module against oracle.librosa_ops on
the CPU and then holds the kernels to it.

  Viterbi   `viterbi_log_dense`: the dense S x S log-transition matrix and librosa's steps; exact (float64 additions and comparisons),
            with `census=True` it counts, on its own `value[t-1] + lt`, the ties a case is meant to force.
  observe   the oracle's `pyin_observations` is the reference; `observe_fsum` restates the trough probabilities by kmin ranks with
            math.fsum (another summation order, to show that the tolerances are not the kernel's), and reports every trough's
            unrounded pitch bin for the near-tie margins.
  LPC       `lpc_formants_exact`: the kernel's float32 Burg recursion with every reduction as the exact sum of the float32 products
            rounded once, the distance of each such sum to a float32 rounding boundary, the float64 response and scipy's peaks."""
import math

import numpy as np
import scipy.signal

from oracle import librosa_ops as L

TINY = float(np.finfo(np.float64).tiny)
VT_THREADS = 1024
VT_MAX_STATES = 2048
SR = 44100
FMIN, FMAX = 65.40639132514966, 2093.004522404789           # C2, C7: the product's pitch range
PRODUCT_BINS, PRODUCT_HALF, PRODUCT_WIDTH = 601, 20, 41       # resolution 0.1, hop 441 at 44.1 kHz: round(35.92 * 12 * 441 / 44100) = 4


# =====================================================================================================================
# Viterbi
# =====================================================================================================================
def dense_log_transition(n_bins, half, lt_same, lt_cross, lt_zero):
    """lt[j, i] = log-transition from source i to DESTINATION j over the 2 n_bins states (voiced block first): the banded tables
    (tap d of destination bin jb <-> source bin jb - half + d; same block -> lt_same, other block -> lt_cross) inside
    |ib - jb| <= half, lt_zero outside.  Table entries whose source bin falls outside 0 .. n_bins - 1 are never used."""
    S, W = 2 * n_bins, 2 * half + 1
    lt_same, lt_cross = np.asarray(lt_same, np.float64), np.asarray(lt_cross, np.float64)
    assert lt_same.shape == lt_cross.shape == (n_bins, W)
    lt = np.full((S, S), float(lt_zero))
    jb = np.broadcast_to(np.arange(n_bins)[:, None], (n_bins, W))
    ib = jb - half + np.arange(W)[None, :]
    ok = (ib >= 0) & (ib < n_bins)
    J, I = jb[ok], ib[ok]
    lt[J, I] = lt_same[ok]
    lt[J + n_bins, I + n_bins] = lt_same[ok]
    lt[J + n_bins, I] = lt_cross[ok]
    lt[J, I + n_bins] = lt_cross[ok]
    return lt


def in_band_mask(n_bins, half):
    b = np.arange(2 * n_bins) % n_bins
    return np.abs(b[:, None] - b[None, :]) <= half


def viterbi_log_dense(logv, logu, n_bins, half, lt_same, lt_cross, lt_zero, log_p_init, census=False):
    """librosa.sequence.viterbi's steps (oracle.librosa_ops.viterbi) on log inputs: value[t-1] + lt, np.argmax (first maximum), add
    log_prob[t], back-track.  logv [T, n_bins], logu [T].  Returns (states [T], ptr [T, S]; row 0 of ptr is not defined) and, with
    `census`, the tie counts (CENSUS_KEYS; see `_count_step` and `_count_max`)."""
    logv, logu = np.asarray(logv, np.float64), np.asarray(logu, np.float64)
    T, S = logv.shape[0], 2 * n_bins
    log_prob = np.concatenate([logv, np.repeat(logu[:, None], n_bins, axis=1)], axis=1)
    lt = dense_log_transition(n_bins, half, lt_same, lt_cross, lt_zero)
    value = np.zeros((T, S))
    ptr = np.zeros((T, S), dtype=np.int64)
    value[0] = log_prob[0] + np.asarray(log_p_init, np.float64)
    counts = _new_census() if census else None
    band = in_band_mask(n_bins, half) if census else None
    rows = np.arange(S)
    for t in range(1, T):
        trans_out = value[t - 1] + lt                                   # [destination j, source i]
        ptr[t] = np.argmax(trans_out, axis=1)
        value[t] = log_prob[t] + trans_out[rows, ptr[t]]
        if census:
            _count_step(counts, trans_out, band, n_bins, value[t - 1])
    states = np.zeros(T, dtype=np.int64)
    states[-1] = np.argmax(value[-1])
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    if census:
        _count_max(counts, value[-1], "final")
        return states, ptr, counts
    return states, ptr


CENSUS_KEYS = ("voiced_unvoiced", "oob_lower", "oob_higher", "oob_wins", "gmax_two_waves", "gmax_two_passes", "gmax_needs_clause",
               "final_tie", "final_needs_clause")


def _new_census():
    return {k: 0 for k in CENSUS_KEYS}


def _count_step(c, trans_out, band, n_bins, prev):
    """Ties of one step, per destination, in the reference's own `value[t-1] + lt`:
      voiced_unvoiced  the maximum is attained by an in-band voiced AND an in-band unvoiced predecessor (the voiced one must win)
      oob_lower / oob_higher  ... by an in-band and an out-of-band predecessor, the first out-of-band index below / above the first
                       in-band one
      oob_wins         the out-of-band predecessor is strictly best (the back-pointer IS the global arg-max)"""
    S = trans_out.shape[0]
    tie = trans_out == trans_out.max(axis=1, keepdims=True)
    voiced = np.arange(S) < n_bins
    tin, tout = tie & band, tie & ~band
    c["voiced_unvoiced"] += int(np.count_nonzero((tin & voiced[None, :]).any(axis=1) & (tin & ~voiced[None, :]).any(axis=1)))
    both = tin.any(axis=1) & tout.any(axis=1)
    fi, fo = np.argmax(tin, axis=1), np.argmax(tout, axis=1)
    c["oob_lower"] += int(np.count_nonzero(both & (fo < fi)))
    c["oob_higher"] += int(np.count_nonzero(both & (fo > fi)))
    c["oob_wins"] += int(np.count_nonzero(~tin.any(axis=1)))
    _count_max(c, prev, "gmax")


def _count_max(c, v, which):
    """Ties of one global arg-max: at two indices in different waves of the 1024-thread reduction, at j and j + 1024 (the two stride
    passes of one thread), and whether the reduction restated WITHOUT its `oi < bi` clause would return another index."""
    idx = np.flatnonzero(v == v.max())
    if which == "final":
        c["final_tie"] += int(len(idx) > 1)
        c["final_needs_clause"] += int(block_argmax_first(v, wave_tie_clause=False) != idx[0])
        return
    c["gmax_two_waves"] += int(len(set(((idx % VT_THREADS) // 64).tolist())) > 1)
    c["gmax_two_passes"] += int(np.intersect1d(idx, idx + VT_THREADS).size > 0)
    c["gmax_needs_clause"] += int(block_argmax_first(v, wave_tie_clause=False) != idx[0])


def block_argmax_first(v, wave_tie_clause=True):
    """The kernel's arg-max reduction restated: each of 1024 threads scans j, j + 1024 (first maximum), each wave of 64 folds with
    shuffle-down steps 32 .. 1 (a lane takes its partner's pair when that is larger, or equal with the lower index), then the 16 wave
    results fold in order.  `wave_tie_clause=False` restates the mutant that drops the equal-value clause of the wave fold: the census
    uses it to show that a case would notice."""
    S = len(v)
    bm = np.full(VT_THREADS, -np.inf)
    bi = np.full(VT_THREADS, 0x7fffffff, dtype=np.int64)
    for start in range(0, S, VT_THREADS):
        seg = v[start:start + VT_THREADS]
        j = start + np.arange(len(seg))
        take = (seg > bm[:len(seg)]) | ((seg == bm[:len(seg)]) & (j < bi[:len(seg)]))
        bm[:len(seg)] = np.where(take, seg, bm[:len(seg)])
        bi[:len(seg)] = np.where(take, j, bi[:len(seg)])
    bm, bi = bm.reshape(16, 64).copy(), bi.reshape(16, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        src = np.where(lane + off < 64, lane + off, lane)
        ov, oi = bm[:, src], bi[:, src]
        take = (ov > bm) | ((ov == bm) & (oi < bi) if wave_tie_clause else False)
        bm, bi = np.where(take, ov, bm), np.where(take, oi, bi)
    gm, gi = bm[0, 0], bi[0, 0]
    for w in range(1, 16):
        if bm[w, 0] > gm or (bm[w, 0] == gm and bi[w, 0] < gi):
            gm, gi = bm[w, 0], bi[w, 0]
    return int(gi)


UNUSED_TAP = 1.0e6           # what the builders put into table entries whose source bin does not exist: it would win if it were read


def _mask_unused(tab, n_bins, half):
    jb = np.arange(n_bins)[:, None]
    ib = jb - half + np.arange(2 * half + 1)[None, :]
    return np.where((ib >= 0) & (ib < n_bins), tab, UNUSED_TAP)


def viterbi_case(kind, n_bins, half, n_frames, seed, plant=()):
    """Inputs of one Viterbi case -> dict(logv, logu, n_bins, half, lt_same, lt_cross, lt_zero, log_p_init).
      product  the product's tables (Context.pyin_transition_tables must be passed in by the caller as `tables`), random observations
      random   random float64 tables in [-10, 0] with lt_zero = -25 (every band entry is above lt_zero, as log(p + tiny) >= log(tiny)
               is in the product: the kernel's single out-of-band candidate relies on it), observations in [-40, 0]
      ties     small integers: tables in {-3 .. 0}, lt_zero = -8, observations in {-6 .. 0} and an all-zero last frame, so that every
               sum is exact and equal sums are real ties; value[0] = log_prob[0] + log_p_init is 0 at the state indices `plant`
               and at most -1 elsewhere, which puts the first global maximum (and, with one frame, the final arg-max) where the
               case wants its ties: in one wave, in two waves, at j and j + 1024
      equal    every observation and table entry 0, lt_zero 0 as well
      equal8   the same with lt_zero = -8 (the lowest in-band index wins instead of index 0)"""
    rng = np.random.default_rng(seed)
    W = 2 * half + 1
    if kind == "random":
        lt_same, lt_cross = rng.uniform(-10, 0, (n_bins, W)), rng.uniform(-10, 0, (n_bins, W))
        lt_zero = -25.0
        logv, logu = rng.uniform(-40, 0, (n_frames, n_bins)), rng.uniform(-40, 0, n_frames)
        lpi = rng.uniform(-5, 0, 2 * n_bins)
    elif kind == "ties":
        lt_same, lt_cross = rng.integers(-3, 1, (n_bins, W)).astype(float), rng.integers(-3, 1, (n_bins, W)).astype(float)
        lt_zero = -8.0
        logv, logu = rng.integers(-6, 1, (n_frames, n_bins)).astype(float), rng.integers(-6, 1, n_frames).astype(float)
        logv[-1], logu[-1] = 0.0, 0.0
        lpi = rng.integers(-2, 0, 2 * n_bins).astype(float)
        if plant:
            logu[0] = 0.0
            for i in plant:
                lpi[i] = 0.0
                if i < n_bins:
                    logv[0, i] = 0.0
    elif kind in ("equal", "equal8"):
        lt_same, lt_cross = np.zeros((n_bins, W)), np.zeros((n_bins, W))
        lt_zero = 0.0 if kind == "equal" else -8.0
        logv, logu, lpi = np.zeros((n_frames, n_bins)), np.zeros(n_frames), np.zeros(2 * n_bins)
    else:
        raise ValueError(kind)
    return dict(logv=logv, logu=logu, n_bins=n_bins, half=half, lt_same=_mask_unused(lt_same, n_bins, half),
                lt_cross=_mask_unused(lt_cross, n_bins, half), lt_zero=lt_zero, log_p_init=lpi)


def product_viterbi_case(tables, n_frames, seed):
    """Random observations in [-40, 0] on the product's layout; `tables` = Context.pyin_transition_tables(601, 41)."""
    half, lt_same, lt_cross, lt_zero, lpi = tables
    rng = np.random.default_rng(seed)
    return dict(logv=rng.uniform(-40, 0, (n_frames, PRODUCT_BINS)), logu=rng.uniform(-40, 0, n_frames), n_bins=PRODUCT_BINS, half=half,
                lt_same=lt_same, lt_cross=lt_cross, lt_zero=lt_zero, log_p_init=lpi)


# (name, kind, n_bins, half, n_frames, seed)
VITERBI_CASES = (
    ("bins1", "random", 1, 0, 16, 1),
    ("bins31", "random", 31, 4, 32, 2),
    ("bins512", "random", 512, 7, 24, 3),
    ("bins513", "random", 513, 7, 24, 4),
    ("bins1024", "random", 1024, 5, 12, 5),
    ("half0", "random", 40, 0, 32, 6),
    ("half_full", "random", 24, 23, 32, 7),
    ("half20_bins21", "random", 21, 20, 32, 8),
    ("one_frame", "random", 40, 3, 1, 9),
    ("two_frames", "random", 40, 3, 2, 10),
    ("one_frame_2048", "random", 1024, 3, 1, 11),
    ("ties_small", "ties", 40, 3, 48, 12),
    ("ties_two_passes", "ties", 600, 4, 24, 13),
    ("ties_2048", "ties", 1024, 2, 12, 14),
    ("ties_one_frame", "ties", 1024, 2, 1, 15),
    ("equal_small", "equal", 40, 3, 8, 0),
    ("equal_2048", "equal", 1024, 2, 4, 0),
    ("equal8_small", "equal8", 40, 3, 8, 0),
    ("equal8_two_passes", "equal8", 600, 20, 4, 0),
)
VITERBI_PLANTS = {"ties_small": (5, 6, 70), "ties_two_passes": (69, 70, 300, 1094), "ties_2048": (69, 70, 300, 1094),
                  "ties_one_frame": (69, 70, 300, 1094)}
# what each forced-tie case must contain at least once (asserted on the reference, without a GPU)
VITERBI_TIES_REQUIRED = {
    "ties_small": ("voiced_unvoiced", "oob_lower", "oob_higher", "oob_wins", "final_tie"),
    "ties_two_passes": ("voiced_unvoiced", "oob_lower", "oob_higher", "oob_wins", "gmax_two_waves", "gmax_two_passes", "gmax_needs_clause",
                        "final_tie"),
    "ties_2048": ("voiced_unvoiced", "oob_lower", "oob_higher", "oob_wins", "gmax_two_waves", "gmax_two_passes", "gmax_needs_clause",
                  "final_tie"),
    "ties_one_frame": ("final_tie", "final_needs_clause"),
}


# =====================================================================================================================
# observation probabilities
# =====================================================================================================================
def fmax_for(n_bins, bps, fmin=FMIN):
    """An fmax for which librosa's floor(12 bps log2(fmax / fmin)) + 1 is n_bins."""
    fmax = fmin * 2.0 ** ((n_bins - 0.5) / (12.0 * bps))
    assert int(np.floor(12 * bps * np.log2(fmax / fmin))) + 1 == n_bins
    return fmax


def observe_ref(launch):
    """The oracle's observations of one launch -> (obs [frames, n_bins], logv, logu, voiced_prob)."""
    with np.errstate(all="ignore"):
        obs, vp, n_bins, bps = L.pyin_observations(np.ascontiguousarray(launch["rows"].T), launch["sr"], launch["fmin"], launch["fmax"],
                                                   launch["min_period"], resolution=1.0 / launch["bps"])
    assert (n_bins, bps) == (launch["n_bins"], launch["bps"])
    obs_v = np.ascontiguousarray(obs[:n_bins].T)
    return obs_v, np.log(obs_v + TINY), np.log((1 - vp) / n_bins + TINY), vp


def observe_fsum(launch):
    """The trough probabilities by kmin ranks (the kernel's formulation: membership of threshold k is monotone in k, so the rank of
    trough j at threshold k is the number of earlier troughs with kmin <= k), every trough's sum taken with math.fsum and the voiced
    mass likewise: the same terms as the oracle's `prior.dot(beta_probs)` in another order.
    Returns (obs [frames, n_bins], voiced_prob, troughs): troughs lists (frame, lag, probability, unrounded bin, bin) of every trough
    with a non-zero probability, in voting order."""
    rows, sr, fmin, min_period = launch["rows"], launch["sr"], launch["fmin"], launch["min_period"]
    n_bins, bps = launch["n_bins"], launch["bps"]
    thresholds, beta_probs = L.pyin_tables()
    F, n_lags = rows.shape
    obs = np.zeros((F, n_bins + 1))
    troughs = []
    for f in range(F):
        c = rows[f]
        tr = L._localmin0(c)
        tr[0] = c[0] < c[1]
        (idx,) = np.nonzero(tr)
        if len(idx) == 0:
            continue
        h = c[idx]
        below = h[:, None] < thresholds[None, 1:]
        kmin = np.where(below.any(axis=1), np.argmax(below, axis=1) + 1, 101)
        terms = [[] for _ in idx]
        for k in range(1, 101):
            member = kmin <= k
            n = int(member.sum())
            if n == 0:
                continue
            fact = (1.0 - np.exp(-2.0)) / (1.0 - np.exp(-2.0 * n))
            rank = np.cumsum(member) - 1
            for j in np.flatnonzero(member):
                terms[j].append(fact * np.exp(-2.0 * rank[j]) * beta_probs[k - 1])
        g = int(np.argmin(h))
        terms[g].append(0.01 * np.sum(beta_probs[:kmin[g] - 1]))
        for j, i in enumerate(idx):
            p = math.fsum(terms[j])
            if p == 0.0:
                continue
            shift = 0.0
            if 0 < i < n_lags - 1:
                with np.errstate(all="ignore"):
                    a = c[i + 1] + c[i - 1] - 2 * c[i]
                    b = (c[i + 1] - c[i - 1]) / 2
                    shift = 0.0 if abs(b) >= abs(a) else -b / a
            raw = 12 * bps * np.log2(sr / (min_period + i + shift) / fmin)
            bi = int(np.clip(np.round(raw), 0, n_bins))
            obs[f, bi] = p
            troughs.append((f, int(i), p, float(raw), bi))
    vp = np.array([min(1.0, max(0.0, math.fsum(obs[f, :n_bins]))) for f in range(F)])
    return obs[:, :n_bins], vp, troughs


def _row(n_lags, base=1.5, **troughs):
    r = np.full(n_lags, float(base))
    for lag, h in troughs.items():
        r[int(lag[1:])] = h
    return r


def _plateau_a0_row(n_lags, lag):
    """A trough whose left neighbour is one ulp above it and whose right neighbour equals it: xp + xm rounds back to 2 x0, so the
    curvature a is exactly 0 while b = -ulp / 2: |b| >= |a| holds and the parabolic shift is suppressed (a true trough has
    a > 0 and |b| <= a / 2 in exact arithmetic, so rounding and +inf are the only ways into that branch)."""
    r = np.full(n_lags, 1.5)
    x0 = 0.25
    r[lag - 1], r[lag], r[lag + 1] = np.nextafter(x0, 1.0), x0, x0
    a = r[lag + 1] + r[lag - 1] - 2 * r[lag]
    b = (r[lag + 1] - r[lag - 1]) / 2
    assert a == 0.0 and b != 0.0 and r[lag] < r[lag - 1]
    r[lag - 2] = 1.5
    return r


def _same_bin_row(n_lags, min_period, sr, fmin, bps):
    """Three troughs two lags apart whose refined periods round into ONE pitch bin: the outer two lean towards the middle one through
    their parabolic shifts.  Returns (row, lags)."""
    lo, mid = 0.2, 0.5
    for i in range(n_lags - 8, 10, -1):
        r = np.full(n_lags, 1.5)
        r[i - 1], r[i], r[i + 1], r[i + 2], r[i + 3], r[i + 4], r[i + 5] = 50.0, lo, mid, lo * 1.01, mid, lo * 1.02, 50.0
        raws = []
        for q in (i, i + 2, i + 4):
            a = r[q + 1] + r[q - 1] - 2 * r[q]
            b = (r[q + 1] - r[q - 1]) / 2
            raws.append(12 * bps * np.log2(sr / (min_period + q - b / a) / fmin))
        if len(set(np.round(raws))) == 1 and all(abs(x - np.floor(x) - 0.5) > 0.02 for x in raws):
            return r, (i, i + 2, i + 4)
    raise AssertionError("no lag puts three troughs into one bin")


def _smooth_rows(n_rows, n_lags, seed):
    """Random smooth curves between about 0 and 1.3 with a handful of troughs at all heights."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_lags) / n_lags
    rows = np.empty((n_rows, n_lags))
    for f in range(n_rows):
        y = np.zeros(n_lags)
        for _ in range(4):
            y += rng.uniform(0.2, 1.0) * np.cos(2 * np.pi * (rng.uniform(1.5, 14.0) * t + rng.uniform()))
        y = (y - y.min()) / (y.max() - y.min())
        rows[f] = rng.uniform(0.0, 0.3) + rng.uniform(0.5, 1.0) * y
    return rows


def observe_launches():
    """Every crafted launch -> list of dict(name, rows [frames, lags], labels, sr, fmin, fmax, min_period, n_bins, bps)."""
    thresholds, _ = L.pyin_tables()
    min_period = max(int(np.floor(SR / FMAX)), 1)
    n_lags = min(int(np.ceil(SR / FMIN)), 2048 - 1024 - 1) - min_period + 1
    prod = dict(sr=float(SR), fmin=FMIN, fmax=FMAX, min_period=min_period, n_bins=PRODUCT_BINS, bps=10)
    rows, labels = [], []

    def add(label, r):
        labels.append(label); rows.append(r)
    add("two_troughs", _row(n_lags, l100=0.05, l300=0.2))
    add("constant", _row(n_lags))                                        # between two frames that have troughs
    add("lag1", _row(n_lags, l1=0.1))
    add("lag0_dropped", _row(n_lags, l0=0.1))                            # period 21: bin 601 = n_bins
    add("lag0_and_more", _row(n_lags, l0=0.1, l200=0.12, l500=0.4))
    add("last_lag", _row(n_lags, **{f"l{n_lags - 1}": 0.1}))
    add("last_lag_and_more", _row(n_lags, **{f"l{n_lags - 1}": 0.1, "l77": 0.3}))
    add("all_high", _row(n_lags, base=3.0, l50=1.0, l200=1.5, l400=2.5))
    for k in (1, 50, 100):
        add(f"on_threshold_{k}", _row(n_lags, l150=thresholds[k], l400=0.35))
        add(f"below_threshold_{k}", _row(n_lags, l150=np.nextafter(thresholds[k], 0.0), l400=0.35))
    add("equal_heights", _row(n_lags, l120=0.07, l380=0.07))
    same, same_lags = _same_bin_row(n_lags, min_period, SR, FMIN, 10)
    add("same_bin3", same)
    add("curvature_zero", _plateau_a0_row(n_lags, 250))
    add("flat_pair", _row(n_lags, l250=0.2, l251=0.2, l420=0.1))
    add("inf_neighbour", _row(n_lags, l200=0.1, l201=np.inf, l202=0.6))
    add("asymmetric", _row(n_lags, l299=0.9, l300=0.15, l301=0.4, l97=0.3, l98=0.25, l99=1.2))
    add("constant_again", _row(n_lags, base=0.4))
    add("two_troughs_again", _row(n_lags, l64=0.33, l611=0.02))
    out = [dict(name="crafted", rows=np.array(rows), labels=labels, same_bin_lags=same_lags, **prod)]
    out.append(dict(name="smooth64", rows=_smooth_rows(64, n_lags, seed=31), labels=[f"smooth{f}" for f in range(64)], **prod))
    # bins below 0 (clamped to 0, later overwrites) and at or above n_bins (dropped), through the caller's min_period
    low = np.array([_row(n_lags, l10=0.1, l300=0.3), _row(n_lags, l5=0.4)])
    out.append(dict(name="clamp_low", rows=low, labels=["two_below_fmin", "one_below_fmin"], **{**prod, "min_period": 700}))
    high = np.array([_row(n_lags, l3=0.1, l8=0.2, l400=0.3), _row(n_lags, l3=0.1), _row(n_lags, l400=0.3, l8=0.05)])
    out.append(dict(name="clamp_high", rows=high, labels=["two_dropped_one_kept", "all_dropped", "minimum_dropped"], **{**prod, "min_period": 1}))
    alt = np.where(np.arange(1024) % 2 == 0, 0.3, 0.7)
    out.append(dict(name="lags1024", rows=np.array([alt, 1.0 - alt, _row(1024, l0=0.2, l1023=0.1)]),
                    labels=["512_troughs_from_lag0", "512_troughs_to_last_lag", "both_ends"], **prod))
    out.append(dict(name="lags1023", rows=np.array([alt[:1023], 1.0 - alt[:1023]]), labels=["512_troughs", "511_troughs"], **prod))
    out.append(dict(name="lags3", rows=np.array([[0.5, 0.2, 0.6], [0.1, 0.5, 0.05], [0.3, 0.3, 0.3], [0.2, 0.5, 0.9], [0.9, 0.5, 0.2]]),
                    labels=["middle", "both_ends", "constant", "first", "last"], **{**prod, "min_period": 100}))
    few = np.array([_row(n_lags, l100=0.05, l300=0.2, l640=0.3), _row(n_lags), _row(n_lags, l0=0.2, l30=0.1), _row(n_lags, l653=0.1, l2=0.4)])
    few_labels = ["three", "constant", "front", "ends"]
    out.append(dict(name="bins1", rows=few, labels=few_labels, **{**prod, "fmax": fmax_for(1, 10), "n_bins": 1}))
    out.append(dict(name="bins1023", rows=few, labels=few_labels, **{**prod, "fmax": fmax_for(1023, 10), "n_bins": 1023, "min_period": 1}))
    out.append(dict(name="bps1", rows=few, labels=few_labels, **{**prod, "bps": 1, "n_bins": int(np.floor(12 * np.log2(FMAX / FMIN))) + 1}))
    return out


# =====================================================================================================================
# LPC formants
# =====================================================================================================================
LP_ORDER_MAX = 32
LP_MAX_FRAME = 2048
LPC_MARGIN_FACTOR = 4.0            # a frame is left out when a reduction lies within 4 n 2^-53 sum|terms| of a float32 rounding boundary
LPC_MAX_LEFT_OUT = 0.02
MAG_BOUND_FACTOR = 64.0 * 2.0 ** -53


def _round_sum_f32(terms32):
    """(float32 of the exact sum of float32 terms, its distance to the nearest float32 rounding boundary, sum of |terms|)."""
    t = terms32.astype(np.float64)
    s = math.fsum(t)
    mag = math.fsum(np.abs(t))
    r = np.float32(s)
    if not np.isfinite(r):
        return r, 0.0, mag
    nz = t[t != 0.0]
    if nz.size == 0:
        return r, np.inf, mag
    # every term is a multiple of q = the float32 spacing at the smallest one; while sum|terms| stays below 2^52 q every partial sum,
    # in any order, is such a multiple below 2^53 q and therefore exact in float64: the kernel's tree sum IS s, whatever the margin
    q = 2.0 ** max(int(np.frexp(np.abs(nz).min())[1]) - 24, -149)
    if mag <= 2.0 ** 52 * q:
        return r, np.inf, mag
    up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    margin = min(abs(s - (float(r) + float(up)) / 2.0), abs(s - (float(r) + float(dn)) / 2.0))
    return r, margin, mag


def burg_exact(frame32, order, preemph):
    """The kernel's Burg recursion on one frame -> (a float32 [order + 1], clear): float32 element-wise arithmetic without
    contraction, each reduction the exact sum of its float32 terms rounded once.  `clear` is False when some reduction lies closer to a
    float32 rounding boundary than LPC_MARGIN_FACTOR * n * 2^-53 * sum|terms| (the kernel's float64 tree sum may then round the
    other way)."""
    f32 = np.float32
    x = np.asarray(frame32, dtype=np.float32)
    with np.errstate(all="ignore"):
        y = np.empty_like(x)
        y[0] = x[0]
        y[1:] = x[1:] - f32(preemph) * x[:-1]
        fwd, bwd = y[1:].copy(), y[:-1].copy()
        ar = np.zeros(order + 1, dtype=np.float32); ar[0] = 1
        ar_prev = ar.copy()
        clear = True

        def reduce(terms):
            nonlocal clear
            r, margin, mag = _round_sum_f32(terms)
            if margin < LPC_MARGIN_FACTOR * len(terms) * 2.0 ** -53 * mag:
                clear = False
            return r
        den = reduce(fwd * fwd + bwd * bwd)
        for it in range(order):
            rc = reduce(bwd * fwd)
            rc = f32(rc * f32(-2.0))
            rc = f32(rc / f32(den + f32(1.17549435e-38)))
            ar_prev, ar = ar, ar_prev
            for j in range(1, it + 2):
                ar[j] = f32(ar_prev[j] + f32(rc * ar_prev[it - j + 1]))
            fwd, bwd = fwd + rc * bwd, bwd + rc * fwd
            q = f32(f32(1.0) - f32(rc * rc))
            den = f32(f32(f32(q * den) - f32(bwd[-1] * bwd[-1])) - f32(fwd[0] * fwd[0]))
            fwd, bwd = fwd[1:], bwd[:-1]
    return ar.copy(), clear


def response_512(a32):
    """1 / |A(e^jw)| at w = pi k / 512, k = 0 .. 511, in float64, with the kernel's arguments w * q."""
    a = np.asarray(a32, dtype=np.float64)
    w = np.pi * np.arange(512, dtype=np.float64) / 512.0
    arg = w[:, None] * np.arange(len(a), dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        re = (a[None, :] * np.cos(arg)).sum(axis=1)
        im = -(a[None, :] * np.sin(arg)).sum(axis=1)
        return 1.0 / np.sqrt(re * re + im * im)


def lpc_formants_exact(x, frame_len, hop, order, preemph, n_frames=None):
    """Per frame: dict(a, finite, clear, count, peaks, mag [3], bound [3], m).  `clear`: the coefficients are pinned (burg_exact) AND every
    peak decision of the reference holds by more than the magnitude bound e[k] = 64 * 2^-53 * sum|a| * m[k]^2: each peak rises above
    both neighbours and clears (or misses) the 10 % height by more than the bound, and no other sample comes within the bound of
    being a peak.  A response that is flat because a[1:] == 0 (1 * cos(0) + 0 + ... = 1 exactly, in any order) is clear, with no peak."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    nf = len(range(0, n - frame_len, hop)) if n_frames is None else n_frames
    out = []
    for f in range(nf):
        a, clear = burg_exact(x[f * hop: f * hop + frame_len], order, preemph)
        rec = dict(a=a, finite=bool(np.all(np.isfinite(a))), clear=clear, count=0, peaks=np.zeros(0, np.int64), mag=np.zeros(3), bound=np.zeros(3), m=None)
        out.append(rec)
        if not rec["finite"] or not a[1:].any():
            continue
        m = response_512(a)
        rec["m"] = m
        if not np.all(np.isfinite(m)):
            rec["finite"] = False
            continue
        e = MAG_BOUND_FACTOR * float(np.abs(a.astype(np.float64)).sum()) * m * m
        hmin = 0.1 * m.max()
        he = 0.1 * e[np.argmax(m)]
        peaks, _ = scipy.signal.find_peaks(m, height=hmin)
        k = np.arange(1, 511)
        rise, fall = m[k] - m[k - 1], m[k] - m[k + 1]
        er, ef = e[k] + e[k - 1], e[k] + e[k + 1]
        is_peak = np.zeros(510, dtype=bool); is_peak[peaks - 1] = True
        sure_peak = (rise > er) & (fall > ef) & (m[k] - hmin > e[k] + he)
        sure_not = (rise < -er) | (fall < -ef) | (m[k] - hmin < -(e[k] + he))
        if not np.all(np.where(is_peak, sure_peak, sure_not)):
            rec["clear"] = False
        rec["count"], rec["peaks"] = len(peaks), peaks
        kk = min(3, len(peaks))
        rec["mag"][:kk], rec["bound"][:kk] = m[peaks[:kk]], e[peaks[:kk]]
    return out


def ar_noise(pole_radii, pole_freqs, n, seed, sr=SR):
    """White noise through 1 / prod (1 - 2 r cos(th) z^-1 + r^2 z^-2), scaled to a peak of 0.5 -> (x float32, pole angles in response bins)."""
    poly = np.array([1.0])
    th = 2 * np.pi * np.asarray(pole_freqs, dtype=np.float64) / sr
    for r, t in zip(pole_radii, th):
        poly = np.convolve(poly, [1.0, -2 * r * np.cos(t), r * r])
    e = np.random.default_rng(seed).standard_normal(n + 4096)
    x = scipy.signal.lfilter([1.0], poly, e)[4096:]
    return (0.5 * x / np.max(np.abs(x))).astype(np.float32), th * 512 / np.pi


def _noise(n, seed, scale=0.2):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def lpc_cases():
    """Every LPC case -> list of dict(name, x, frame_len, hop, order, preemph [, poles: pole angles in response bins]).  At most 64
    frames each; the frame count is the wrapper's len(range(0, n - frame_len, hop))."""
    from audio_cut_amd.testing import signals
    voice = signals.voice_with_rests(2.0, seed=4)[2000:]
    fl, hop = 1102, 441

    def span(frames, frame_len=fl, h=hop):
        return frame_len + (frames - 1) * h + 1
    cases = [dict(name="voice_order12", x=voice[:span(64)], frame_len=fl, hop=hop, order=12, preemph=0.95)]
    x4, p4 = ar_noise((0.999, 0.997), (3000.0, 9000.0), span(24, 2048, 512), seed=3)
    cases.append(dict(name="ar4", x=x4, frame_len=2048, hop=512, order=4, preemph=0.0, poles=p4))
    x8, p8 = ar_noise((0.999, 0.997, 0.997, 0.997), (3000.0, 7000.0, 12000.0, 17000.0), span(24, 2048, 512), seed=5)
    cases.append(dict(name="ar8_four_peaks", x=x8, frame_len=2048, hop=512, order=8, preemph=0.0, poles=p8))
    cases.append(dict(name="order1", x=voice[:span(64)], frame_len=fl, hop=hop, order=1, preemph=0.95))
    cases.append(dict(name="order32", x=voice[:span(48)], frame_len=fl, hop=hop, order=32, preemph=0.95))
    cases.append(dict(name="len4_order1", x=_noise(span(64, 4, 3), 11), frame_len=4, hop=3, order=1, preemph=0.95))
    cases.append(dict(name="len4_order2", x=_noise(span(64, 4, 3), 12), frame_len=4, hop=3, order=2, preemph=0.95))
    for frame_len in (255, 256, 257):
        cases.append(dict(name=f"len{frame_len}", x=voice[:span(32, frame_len)], frame_len=frame_len, hop=hop, order=12, preemph=0.95))
    cases.append(dict(name="len2048_order12", x=voice[:span(16, 2048)], frame_len=2048, hop=hop, order=12, preemph=0.95))
    cases.append(dict(name="len2048_order32", x=voice[:span(16, 2048)], frame_len=2048, hop=hop, order=32, preemph=0.95))
    cases.append(dict(name="hop_divides", x=voice[:fl + 5 * hop], frame_len=fl, hop=hop, order=12, preemph=0.95))          # 5 frames
    cases.append(dict(name="hop_divides_plus_1", x=voice[:fl + 5 * hop + 1], frame_len=fl, hop=hop, order=12, preemph=0.95))  # 6 frames
    z = voice[:span(16)].copy()
    z[3 * hop: 6 * hop + fl] = 0.0                                                                # frames 3 .. 6 are all zero
    cases.append(dict(name="zero_frames", x=z, frame_len=fl, hop=hop, order=12, preemph=0.95))
    t = np.arange(span(3)) / SR
    cases.append(dict(name="constant", x=np.full(span(3), 0.25, np.float32), frame_len=fl, hop=hop, order=12, preemph=0.95))
    imp = np.zeros(span(3), np.float32); imp[900] = 0.5
    cases.append(dict(name="impulse", x=imp, frame_len=fl, hop=hop, order=12, preemph=0.95))
    cases.append(dict(name="sinusoid", x=(0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32), frame_len=fl, hop=hop, order=12, preemph=0.95))
    return cases
