"""The pitch kernels (audio_cut_amd/csrc/ac_pitch.hip) stage by stage, on crafted inputs, against tests/pitch_refs.py.

  ac_pyin_viterbi   BIT-EXACT.  Given logv / logu the kernel only adds and compares float64, so `states` and rows 1 .. of the
                    back-pointer table equal the dense S x S reference (librosa's steps, np.argmax's first maximum) exactly: the
                    product layout, 2 .. 2048 states, bands of 0 .. n_bins - 1, integer inputs whose ties are real (counted on the
                    reference first), all-equal inputs, one and two frames.
  ac_pyin_observe   against oracle.librosa_ops.pyin_observations in float64 on hand-built CMND rows.  A trough probability is a sum of
                    at most 100 positive products, so two summation orders differ by at most about 100 * 2^-53 = 1.1e-14 relative:
                      voiced_prob  rtol 1e-12                       largest observed 1.1e-15 (math.fsum restatement on the host: 5.6e-16)
                      logv, logu   atol 1e-12 + 4 ulp(|reference|)  largest observed 4.5e-14 on occupied bins and logu, 0 on
                                   the empty bins, where it is the device's log(tiny) (math.fsum restatement: 7.2e-15 and 0)
                      empty bins   the same set: reference 0  <=>  logv < -700 (see _check_observe for the 512-trough rows, whose
                                   late votes underflow below e^-700)
                    The pitch bin of a trough is a rounding decision; test_observe_inputs_stay_clear_of_near_ties keeps every
                    crafted trough 1e-6 of a bin away from it (the closest is 3.7e-4).
  ac_lpc_formants   the Burg recursion BIT FOR BIT, then the response in float64.  pitch_refs.burg_exact states the kernel's float32
                    arithmetic with each reduction as the exact sum of its float32 terms rounded once; the kernel's float64 tree sum
                    rounds to the same float32 unless the exact sum lies within n 2^-53 sum|terms| of a rounding boundary, and
                    frames within 4 times that are left out (at most 2 % of a case: test_lpc_cases_leave_out_at_most_2_percent; with
                    the cases below, none).  With equal coefficients a_q only the evaluation of A(w) = sum_q a_q e^(-j w q) differs:
                    each of the <= 33 products and additions of the real and of the imaginary part errs by at most 2^-53 of a partial
                    sum <= sum|a_q|, sincos by a few ulp of values <= 1, so |dA| <= 64 * 2^-53 * sum|a_q| with room, and to first
                    order d(1 / |A|) = |dA| / |A|^2:
                      |mag - reference| <= 64 * 2^-53 * sum_q|a_q| * mag^2      largest observed error / bound 0.021
                    A float32 coefficient off by one bit moves a magnitude near a pole by about 6e-8 sum|a| mag, orders above this
                    bound.  Peak counts are exact wherever every peak decision of the reference is clear by more than the bound.

One-token mutations of a scratch copy of ac_pitch.hip, built and run on an MI355X, and the cases of this module that failed:
  band loop `v >= best` for `v > best`           test_viterbi_bit_exact: ties_small, ties_two_passes, ties_2048, equal8_small,
                                                 equal8_two_passes, product64, product400 (the triangle's symmetric taps tie too)
  wave fold without its `oi < bi` clause         test_viterbi_bit_exact: ties_two_passes, ties_2048, ties_one_frame
  `s_obs[bi] += p` for `= p`                     test_observe_crafted_rows: crafted, clamp_low, lags1024, lags1023
  `h <= thresholds[k]` for `h < thresholds[k]`   test_observe_crafted_rows: every launch but smooth64
  rc divided by the s_den of one iteration ago   test_lpc_formants_exact: the 16 cases of order 2 and more
  `it - tid` for `it - tid + 1` in the s_ar update   test_lpc_formants_exact: the 16 cases of order 2 and more
(at order 1 the last two mutants compute the same as the kernel: order1 and len4_order1 pass them, rightly)"""
import functools

import numpy as np
import pytest
import torch

import pitch_refs as P
from audio_cut_amd import _native
from audio_cut_amd.testing import signals
from oracle import librosa_ops as L

SR = P.SR
VP_RTOL = 1e-12
LOG_ATOL, LOG_ULPS = 1e-12, 4
BIN_MARGIN = 1e-6
SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------------------------------------
# shared, cached case data (computed once per session, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _product_tables():
    return _native.Context.pyin_transition_tables(P.PRODUCT_BINS, P.PRODUCT_WIDTH, 0.01)


VITERBI_IDS = [c[0] for c in P.VITERBI_CASES] + ["product64", "product400"]


@functools.lru_cache(maxsize=None)
def _viterbi_case(name):
    """(inputs, states, ptr, census or None) of one case."""
    if name.startswith("product"):
        case = P.product_viterbi_case(_product_tables(), int(name[7:]), seed=len(name))
        return (case,) + P.viterbi_log_dense(**case) + (None,)
    _, kind, n_bins, half, n_frames, seed = next(c for c in P.VITERBI_CASES if c[0] == name)
    case = P.viterbi_case(kind, n_bins, half, n_frames, seed, P.VITERBI_PLANTS.get(name, ()))
    if kind == "ties":
        return (case,) + P.viterbi_log_dense(**case, census=True)
    return (case,) + P.viterbi_log_dense(**case) + (None,)


@functools.lru_cache(maxsize=None)
def _launches():
    return {l["name"]: l for l in P.observe_launches()}


@functools.lru_cache(maxsize=None)
def _observe_refs(name):
    l = _launches()[name]
    return P.observe_ref(l), P.observe_fsum(l)


@functools.lru_cache(maxsize=None)
def _lpc_cases():
    return {c["name"]: c for c in P.lpc_cases()}


@functools.lru_cache(maxsize=None)
def _lpc_ref(name):
    c = _lpc_cases()[name]
    return P.lpc_formants_exact(c["x"], c["frame_len"], c["hop"], c["order"], c["preemph"])


OBSERVE_IDS = ["crafted", "smooth64", "clamp_low", "clamp_high", "lags1024", "lags1023", "lags3", "bins1", "bins1023", "bps1"]
LPC_IDS = ["voice_order12", "ar4", "ar8_four_peaks", "order1", "order32", "len4_order1", "len4_order2", "len255", "len256", "len257",
           "len2048_order12", "len2048_order32", "hop_divides", "hop_divides_plus_1", "zero_frames", "constant", "impulse", "sinusoid"]


def test_case_lists_are_complete():
    assert OBSERVE_IDS == list(_launches()) and LPC_IDS == list(_lpc_cases())


# ---------------------------------------------------------------------------------------------------------------------
# host: the references against the oracle, the ties, the margins, the caps
# ---------------------------------------------------------------------------------------------------------------------
def _voice_observations():
    x = signals.voice_with_rests(1.0, seed=6)
    cm, min_period, _ = L.cmnd_frames(x, SR, P.FMIN, P.FMAX, 2048, 441)
    obs, vp, n_bins, bps = L.pyin_observations(cm, SR, P.FMIN, P.FMAX, min_period)
    assert (n_bins, bps) == (P.PRODUCT_BINS, 10)
    return obs, vp


def test_dense_viterbi_matches_the_oracle_on_a_voice_clip():
    """Product tables from Context.pyin_transition_tables + the dense reference on log observations == oracle.librosa_ops.viterbi on
    the probabilities (its own dense kron transition matrix), state for state; the clip has voiced and unvoiced stretches."""
    obs, _ = _voice_observations()
    n_bins = P.PRODUCT_BINS
    half, lt_same, lt_cross, lt_zero, lpi = _product_tables()
    assert half == P.PRODUCT_HALF and lt_same.shape == (n_bins, 2 * half + 1)
    transition = np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), L.transition_local_triangle(n_bins, P.PRODUCT_WIDTH))
    p_init = np.zeros(2 * n_bins); p_init[n_bins:] = 1 / n_bins
    ref = L.viterbi(obs, transition, p_init)
    assert 0.1 < np.mean(ref < n_bins) < 0.9
    # the banded tables ARE the oracle's dense matrix
    dense = P.dense_log_transition(n_bins, half, lt_same, lt_cross, lt_zero)
    assert np.array_equal(dense, np.log(transition + P.TINY).T)
    logp = np.log(obs.T + P.TINY)
    assert np.all(logp[:, n_bins:] == logp[:, n_bins:n_bins + 1])
    states, _ = P.viterbi_log_dense(logp[:, :n_bins], logp[:, n_bins], n_bins, half, lt_same, lt_cross, lt_zero, lpi)
    assert np.array_equal(states, ref)


def test_block_argmax_restatement_returns_the_first_maximum():
    rng = np.random.default_rng(0)
    for S in (2, 62, 80, 1024, 1026, 1200, 2048):
        for _ in range(5):
            v = rng.integers(-3, 1, S).astype(float)
            assert P.block_argmax_first(v) == int(np.argmax(v)), S


@pytest.mark.parametrize("name", sorted(P.VITERBI_TIES_REQUIRED))
def test_forced_tie_cases_contain_their_ties(name):
    """Counted on the reference's own `value[t-1] + lt`, per destination and step: each kind of tie the case is there for occurs."""
    case, states, ptr, census = _viterbi_case(name)
    for a in (case["logv"], case["logu"], case["log_p_init"]):
        assert np.array_equal(a, np.round(a))
    print(name, census)
    for key in P.VITERBI_TIES_REQUIRED[name]:
        assert census[key] > 0, (name, key, census)


def test_all_equal_reference_points_at_the_lowest_admissible_index():
    for name in ("equal_small", "equal8_small"):
        case, states, ptr, _ = _viterbi_case(name)
        n_bins, half = case["n_bins"], case["half"]
        jb = np.arange(2 * n_bins) % n_bins
        want = np.zeros(2 * n_bins, np.int64) if name == "equal_small" else np.maximum(jb - half, 0)
        assert np.all(ptr[1:] == want[None, :]) and np.all(states == 0)


def _log_close(got, ref):
    """|got - ref| <= 1e-12 + 4 ulp(|ref|), element by element -> largest difference."""
    diff = np.abs(got - ref)
    bad = diff > LOG_ATOL + LOG_ULPS * np.spacing(np.abs(ref))
    assert not bad.any(), f"first at {np.argwhere(bad)[0]}: got {got[bad][0]!r}, reference {ref[bad][0]!r}"
    return float(diff.max()) if diff.size else 0.0


def _check_observe(name, logv, logu, vp):
    """The comparison of the issue, shared by the GPU test and the host restatement -> (max |dlog| on occupied bins and logu,
    max |dlog| on empty bins, max relative voiced_prob difference)."""
    (obs, rlv, rlu, rvp), _ = _observe_refs(name)
    assert logv.shape == rlv.shape and logu.shape == rlu.shape and vp.shape == rvp.shape
    empty = rlv < -700.0
    # reference 0 <=> logv < -700.  Only the 512-trough rows hold votes that are not 0 and yet below e^-700 (a Boltzmann rank
    # beyond 345: e^-690 and less, down to denormals): there "empty" is read off the reference's own logarithm, which log(p + tiny)
    # cannot tell from an empty bin at any tolerance; everywhere else the two readings are the same set, asserted here.
    if not name.startswith("lags102"):
        assert np.array_equal(empty, obs == 0.0), name
    assert np.all(empty[obs == 0.0])
    assert np.array_equal(empty, logv < -700.0), f"{name}: empty bins differ, first at {np.argwhere(empty != (logv < -700.0))[0]}"
    d_occ = max(_log_close(logv[~empty], rlv[~empty]), _log_close(logu, rlu))
    d_empty = _log_close(logv[empty], rlv[empty])
    dv = np.abs(vp - rvp)
    assert np.all(dv <= VP_RTOL * np.abs(rvp)), f"{name}: voiced_prob {vp[np.argmax(dv)]!r} against {rvp[np.argmax(dv)]!r}"
    rel = float(np.max(dv[rvp > 0] / rvp[rvp > 0])) if (rvp > 0).any() else 0.0
    return d_occ, d_empty, rel


@pytest.mark.parametrize("name", OBSERVE_IDS)
def test_observe_bounds_hold_for_another_summation_order(name):
    """The rank formulation with math.fsum per trough (pitch_refs.observe_fsum) against the oracle, held to the SAME bounds as the
    kernel: the bounds are a property of the operation, not of the kernel's order of summation."""
    _, (obs, vp, _) = _observe_refs(name)
    l = _launches()[name]
    with np.errstate(divide="ignore"):
        figures = _check_observe(name, np.log(obs + P.TINY), np.log((1 - vp) / l["n_bins"] + P.TINY), vp)
    print(name, "fsum restatement: max dlog occupied %.3e, empty %.3e, voiced_prob rel %.3e" % figures)


def test_observe_inputs_stay_clear_of_near_ties():
    """rint(12 bps log2(f0 / fmin)) may flip on a last-ulp difference of log2.  Every crafted trough that votes keeps its unrounded
    bin at least 1e-6 away from a half-integer, which covers the clamp edges as well (the clamps act on the rounded value: they
    switch at -0.5 and at n_bins - 0.5 / n_bins + 0.5).  No trough is excluded."""
    closest = 1.0
    for name in OBSERVE_IDS:
        _, (_, _, troughs) = _observe_refs(name)
        assert troughs, name
        raw = np.array([t[3] for t in troughs])
        dist = np.abs(raw - np.floor(raw) - 0.5)
        assert dist.min() >= BIN_MARGIN, (name, troughs[int(np.argmin(dist))])
        closest = min(closest, float(dist.min()))
    print("closest unrounded bin to a half-integer: %.3e" % closest)


def test_observe_cases_reach_their_branches():
    """What each crafted row is there for, asserted on the references (no GPU)."""
    thresholds, beta_probs = L.pyin_tables()
    l = _launches()["crafted"]
    (obs, _, _, vp), (_, _, troughs) = _observe_refs("crafted")
    row = {lab: f for f, lab in enumerate(l["labels"])}
    by_frame = lambda lab: [t for t in troughs if t[0] == row[lab]]
    n_lags = l["rows"].shape[1]
    for lab in ("constant", "constant_again"):                          # no trough at all, between frames that have some
        assert vp[row[lab]] == 0.0 and not obs[row[lab]].any() and not by_frame(lab)
        assert by_frame(l["labels"][row[lab] - 1]) and by_frame(l["labels"][row[lab] + 1])
    assert [t[1] for t in by_frame("lag1")] == [1]
    assert [(t[1], t[4]) for t in by_frame("lag0_dropped")] == [(0, l["n_bins"])] and vp[row["lag0_dropped"]] == 0.0
    assert by_frame("lag0_and_more")[0][1] == 0 and vp[row["lag0_and_more"]] > 0.0
    assert [t[1] for t in by_frame("last_lag")] == [n_lags - 1] and by_frame("last_lag_and_more")[-1][1] == n_lags - 1
    # heights >= 1: kmin = 101 everywhere, only the global minimum (lag 50) takes no_trough_prob * sum(beta_probs)
    assert [t[1] for t in by_frame("all_high")] == [50]
    assert vp[row["all_high"]] == pytest.approx(0.01 * np.sum(beta_probs), rel=1e-14)
    # on / just below thresholds[k]: the trough joins threshold k only below it
    for k in (1, 50, 100):
        on, below = row[f"on_threshold_{k}"], row[f"below_threshold_{k}"]
        assert l["rows"][on, 150] == thresholds[k] and l["rows"][below, 150] < thresholds[k]
        # (beta_probs[99] = cdf(1) - cdf(0.99) of Beta(2, 18) is exactly 0 in float64: at k = 100 both rows must give the same, no vote)
        assert np.array_equal(obs[on], obs[below]) == (beta_probs[k - 1] == 0.0), k
    assert beta_probs[0] > 0.0 and beta_probs[49] > 0.0 and beta_probs[99] == 0.0
    assert not [t for t in by_frame("on_threshold_100") + by_frame("below_threshold_100") if t[1] == 150]
    eq = by_frame("equal_heights")
    assert len(eq) == 2 and eq[0][2] > eq[1][2]                        # the first of two equal troughs is the global minimum
    same = by_frame("same_bin3")
    assert [t[1] for t in same] == list(l["same_bin_lags"]) and len({t[4] for t in same}) == 1
    assert vp[row["same_bin3"]] < 0.5 * sum(t[2] for t in same)        # later overwrites: the sum would be more than twice as large
    assert vp[row["same_bin3"]] == pytest.approx(same[-1][2], rel=1e-12)
    r = l["rows"][row["curvature_zero"]]
    assert r[251] + r[249] - 2 * r[250] == 0.0 and abs((r[251] - r[249]) / 2) > 0.0      # a == 0, |b| >= |a|
    cz = [t for t in by_frame("curvature_zero") if t[1] == 250]
    assert cz and cz[0][3] == 12 * 10 * np.log2(SR / (l["min_period"] + 250.0) / P.FMIN)
    assert np.isinf(l["rows"][row["inf_neighbour"], 201]) and [t[1] for t in by_frame("inf_neighbour")] == [200, 202]
    # clamps through the caller's min_period
    for name, edge in (("clamp_low", 0), ("clamp_high", P.PRODUCT_BINS)):
        _, (_, _, tr) = _observe_refs(name)
        hit = [t for t in tr if t[4] == edge]
        assert hit and all(t[3] < -1.0 if edge == 0 else t[3] > edge + 1.0 for t in hit), name
    (_, _, _, vph), (_, _, trh) = _observe_refs("clamp_high")
    assert vph[1] == 0.0 and vph[2] == pytest.approx([t[2] for t in trh if t[0] == 2 and t[1] == 400][0], rel=1e-12)
    # 512 troughs: the capacity of the trough list and of the Boltzmann tables
    for name, counts in (("lags1024", (512, 512, 2)), ("lags1023", (512, 511))):
        rows = _launches()[name]["rows"]
        for f, c in enumerate(counts):
            tr = L._localmin0(rows[f]); tr[0] = rows[f, 0] < rows[f, 1]
            assert tr.sum() == c, (name, f)
    assert _launches()["bins1"]["n_bins"] == 1 and _launches()["bins1023"]["n_bins"] == 1023 and _launches()["bps1"]["bps"] == 1


def test_lpc_exact_reference_matches_the_oracle_chain():
    """pitch_refs.lpc_formants_exact against L.lpc + freqz + find_peaks (the reference of test_lpc_formants_edges) at that test's
    rtol 5e-3, equal counts, on a voice clip."""
    import scipy.signal as signal
    frame_len, hop = 1102, 441
    x = signals.voice_with_rests(2.0, seed=4)[: frame_len + 40 * hop]
    ref = P.lpc_formants_exact(x, frame_len, hop, 12, 0.95)
    assert len(ref) == 40
    for f, rec in enumerate(ref):
        fr = x[f * hop: f * hop + frame_len]
        fr = np.append(fr[0], fr[1:] - 0.95 * fr[:-1])
        _, h = signal.freqz(1, L.lpc(fr, 12), worN=512, fs=SR)
        m = np.abs(h)
        peaks, _ = signal.find_peaks(m, height=np.max(m) * 0.1)
        assert rec["count"] == len(peaks), f
        k = min(3, len(peaks))
        np.testing.assert_allclose(rec["mag"][:k], m[peaks[:k]], rtol=5e-3, atol=1e-6, err_msg=str(f))


@pytest.mark.parametrize("name", LPC_IDS)
def test_lpc_cases_leave_out_at_most_2_percent(name):
    """Frames whose reductions come too close to a float32 rounding boundary, or whose peak decisions are not clear by more than the
    magnitude bound, are not compared; the chosen inputs need that for at most 2 % of a case's frames.  No case produces a
    non-finite coefficient (the collapsing denominators of constant / impulse / sinusoid included), so every case is compared."""
    c, ref = _lpc_cases()[name], _lpc_ref(name)
    assert 1 <= len(ref) <= 64
    assert all(r["finite"] for r in ref)
    left_out = sum(not r["clear"] for r in ref)
    assert left_out <= P.LPC_MAX_LEFT_OUT * len(ref), (name, left_out, len(ref))
    counts = [r["count"] for r in ref]
    if "poles" in c:                                                    # sharp poles at known angles: every peak within one response bin
        assert all(r["count"] == len(c["poles"]) for r in ref)
        assert max(np.abs(np.sort(r["peaks"]) - np.sort(c["poles"])).max() for r in ref) <= 1.0
    if name == "ar8_four_peaks":
        assert min(counts) > 3
    if name == "zero_frames":
        zero = [f for f in range(len(ref)) if not c["x"][f * c["hop"]: f * c["hop"] + c["frame_len"]].any()]
        assert len(zero) >= 3 and all(ref[f]["count"] == 0 and not ref[f]["a"][1:].any() for f in zero) and max(counts) > 0
    if name in ("hop_divides", "hop_divides_plus_1"):
        assert len(ref) == (5 if name == "hop_divides" else 6)
    if name in ("voice_order12", "order32"):
        assert max(counts) > 3


# ---------------------------------------------------------------------------------------------------------------------
# GPU: ac_pyin_viterbi
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", VITERBI_IDS)
def test_viterbi_bit_exact(hip_ctx, name):
    case, ref_states, ref_ptr, _ = _viterbi_case(name)
    T, S = case["logv"].shape[0], 2 * case["n_bins"]
    states, ptr = hip_ctx.pyin_viterbi(hip_ctx.to_device(case["logv"]), hip_ctx.to_device(case["logu"]), case["n_bins"], case["half"],
                                       case["lt_same"], case["lt_cross"], case["lt_zero"], case["log_p_init"])
    assert states.shape == (T,) and ptr.shape == (T, S)
    states = states.cpu().numpy().astype(np.int64)
    assert np.array_equal(states, ref_states), f"{name}: first state difference at frame {int(np.argmax(states != ref_states))}"
    if T > 1:                                                           # row 0 is never written
        got = ptr.cpu().numpy().view(np.uint16)[1:].astype(np.int64)
        bad = got != ref_ptr[1:]
        assert not bad.any(), f"{name}: {int(bad.sum())} back-pointers differ, first at (t, j) = {tuple(np.argwhere(bad)[0] + [1, 0])}"


@pytest.mark.gpu
def test_viterbi_wrapper_refuses_tables_of_another_shape(hip_ctx, monkeypatch):
    """The kernel reads the tables by n_bins and half: the wrapper does not pass on a buffer of another shape."""
    case = dict(_viterbi_case("half0")[0])
    logv, logu = hip_ctx.to_device(case["logv"]), hip_ctx.to_device(case["logu"])
    monkeypatch.setattr(hip_ctx.lib, "ac_pyin_viterbi", lambda *a: pytest.fail("ac_pyin_viterbi called"), raising=False)
    for key, bad in (("lt_same", case["lt_same"][:-1]), ("lt_cross", case["lt_cross"][:, :0]), ("log_p_init", case["log_p_init"][1:]),
                     ("half", 1)):
        args = {**case, key: bad}
        with pytest.raises(_native.NativeError, match="pyin_viterbi"):
            hip_ctx.pyin_viterbi(logv, logu, args["n_bins"], args["half"], args["lt_same"], args["lt_cross"], args["lt_zero"], args["log_p_init"])
    with pytest.raises(_native.NativeError, match="pyin_viterbi"):
        hip_ctx.pyin_viterbi(logv[:, :-1].contiguous(), logu, case["n_bins"], case["half"], case["lt_same"], case["lt_cross"], case["lt_zero"],
                             case["log_p_init"])


def _viterbi_direct(hip_ctx, n_frames, n_bins, half, rows=4, bins=64, width=7):
    """A direct call with generously sized, sentinel-filled buffers -> (return code, states, ptr)."""
    dev = hip_ctx.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    logv, logu, lt_same, lt_cross, lpi = z(rows, bins), z(rows), z(bins, width), z(bins, width), z(2 * bins)
    states = torch.full((rows,), -77, dtype=torch.int32, device=dev)
    ptr = torch.full((rows, 2 * bins), -77, dtype=torch.int16, device=dev)
    rc = hip_ctx.lib.ac_pyin_viterbi(hip_ctx._h, logv.data_ptr(), logu.data_ptr(), n_frames, n_bins, half, lt_same.data_ptr(),
                                     lt_cross.data_ptr(), -8.0, lpi.data_ptr(), ptr.data_ptr(), states.data_ptr(), _native._stream())
    torch.cuda.synchronize()
    return rc, states, ptr


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,n_bins,half,cause", [(4, 1025, 2, "2 * n_bins <= VT_MAX_STATES"), (4, 40, 40, "half < n_bins"),
                                                         (4, 40, -1, "half >= 0"), (0, 40, 3, "n_frames > 0"), (4, 0, 0, "n_bins >= 1")])
def test_viterbi_refusals_come_before_any_launch(hip_ctx, n_frames, n_bins, half, cause):
    rc, states, ptr = _viterbi_direct(hip_ctx, n_frames, n_bins, half)
    assert rc != 0
    with pytest.raises(_native.NativeError, match="state layout") as e:
        _native._check(rc)
    assert cause in str(e.value)
    assert bool((states == -77).all()) and bool((ptr == -77).all())
    rc, states, _ = _viterbi_direct(hip_ctx, 4, 40, 3)                  # the same buffers are fine for an admitted layout
    assert rc == 0 and bool((states == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: ac_pyin_observe
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OBSERVE_IDS)
def test_observe_crafted_rows(hip_ctx, name):
    """One launch per layout, one frame per case: every block sees another trough count."""
    l = _launches()[name]
    logv, logu, vp = hip_ctx.pyin_observe(hip_ctx.to_device(l["rows"]), l["sr"], l["fmin"], l["min_period"], l["n_bins"], l["bps"])
    figures = _check_observe(name, logv.cpu().numpy(), logu.cpu().numpy(), vp.cpu().numpy())
    print(name, "kernel: max dlog occupied %.3e, empty %.3e, voiced_prob rel %.3e" % figures)


@pytest.mark.gpu
@pytest.mark.parametrize("n_lags,n_bins,min_period,cause", [(2, 601, 21, "n_lags >= 3"), (1025, 601, 21, "n_lags <= PY_MAX_LAGS"),
                                                             (655, 0, 21, "n_bins >= 1"), (655, 1024, 21, "n_bins < 1024"),
                                                             (655, 601, 0, "min_period >= 1")])
def test_observe_refusals_come_before_any_launch(hip_ctx, n_lags, n_bins, min_period, cause):
    dev = hip_ctx.device
    cmnd = torch.full((4, 1025), 0.5, dtype=torch.float64, device=dev)
    tabs = [hip_ctx.to_device(np.ascontiguousarray(t, dtype=np.float64)) for t in hip_ctx._pyin_tables()]
    logv = torch.full((4, 1024), SENTINEL, dtype=torch.float64, device=dev)
    logu = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev)
    vp = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev)
    rc = hip_ctx.lib.ac_pyin_observe(hip_ctx._h, cmnd.data_ptr(), 4, n_lags, min_period, float(SR), P.FMIN, n_bins, 10,
                                     *[t.data_ptr() for t in tabs], 0.01, P.TINY, logv.data_ptr(), logu.data_ptr(), vp.data_ptr(),
                                     _native._stream())
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_native.NativeError, match="invalid argument") as e:
        _native._check(rc)
    assert cause in str(e.value)
    assert bool((logv == SENTINEL).all()) and bool((logu == SENTINEL).all()) and bool((vp == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: ac_lpc_formants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", LPC_IDS)
def test_lpc_formants_exact(hip_ctx, name):
    c, ref = _lpc_cases()[name], _lpc_ref(name)
    cnt, mag = hip_ctx.lpc_formants(hip_ctx.to_device(c["x"]), c["frame_len"], c["hop"], order=c["order"], preemph=c["preemph"])
    assert cnt.shape == (len(ref),) and mag.shape == (len(ref), 3)
    worst, compared = 0.0, 0
    for f, r in enumerate(ref):
        if not r["clear"]:
            continue
        compared += 1
        assert cnt[f] == r["count"], (name, f, int(cnt[f]), r["count"])
        k = min(3, r["count"])
        assert np.all(mag[f, k:] == 0.0), (name, f)
        if k:
            err = np.abs(mag[f, :k] - r["mag"][:k])
            worst = max(worst, float(np.max(err / r["bound"][:k])))
            assert np.all(err <= r["bound"][:k]), (name, f, mag[f, :k].tolist(), r["mag"][:k].tolist(), r["bound"][:k].tolist())
    assert compared >= (1.0 - P.LPC_MAX_LEFT_OUT) * len(ref)
    print(name, "frames compared %d of %d, worst error / bound %.3f" % (compared, len(ref), worst))


@pytest.mark.gpu
@pytest.mark.parametrize("n,frame_len,hop,order,n_frames,cause", [
    (5000, 4, 3, 3, 4, "order < frame_len - 1"), (5000, 4, 3, 2, 0, "n_frames > 0"), (5000, 1102, 441, 0, 4, "order >= 1"),
    (5000, 1102, 441, 33, 4, "order <= LP_ORDER_MAX"), (5000, 3, 3, 1, 4, "frame_len >= 4"), (5000, 2049, 441, 12, 4, "frame_len <= LP_MAX_FRAME"),
    (1102 + 3 * 441 - 1, 1102, 441, 12, 4, "frames must lie inside the signal"), (1102, 1102, 441, 12, 2, "frames must lie inside the signal"),
    (5000, 1102, 441, 12, 0, "n_frames > 0")])
def test_lpc_refusals_come_before_any_launch(hip_ctx, n, frame_len, hop, order, n_frames, cause):
    dev = hip_ctx.device
    x = torch.full((8192,), 0.25, dtype=torch.float32, device=dev)
    cnt = torch.full((8,), -77, dtype=torch.int32, device=dev)
    mag = torch.full((8, 3), SENTINEL, dtype=torch.float64, device=dev)
    rc = hip_ctx.lib.ac_lpc_formants(hip_ctx._h, x.data_ptr(), n, frame_len, hop, order, 0.95, cnt.data_ptr(), mag.data_ptr(), n_frames,
                                     _native._stream())
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_native.NativeError, match="invalid argument") as e:
        _native._check(rc)
    assert cause in str(e.value)
    assert bool((cnt == -77).all()) and bool((mag == SENTINEL).all())
