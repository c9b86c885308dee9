"""CPU checks of tests/resample_refs.py, the float64 same-taps reference the GPU tests of the polyphase resamplers rest on
(tests/test_resample_pcm_edges_gpu.py): it is scipy.signal.resample_poly when scipy is given the same taps, its impulse train
reads every tap once, its comparisons reject three off-by-one mutants of the kernel's index arithmetic on the GPU tests' own case
table, and the hand-derived PCM words of the GPU tests are what the host conversion gives."""
import math

import numpy as np
import pytest

import resample_refs as R
import test_resample_pcm_edges_gpu as G
from audio_cut_amd.utils.audio_export import pcm_bytes_host

SIX = [(147, 160), (160, 441), (2, 1), (1, 2), (3, 7), (7, 3)]


def _scipy_window(hfull, up, down, n_pre_remove):
    """`Context._resample_filter` returns scipy's framing (front-padded by n_pre_pad zeros, scaled by up); scipy wants the bare odd
    filter at unit gain and applies that framing itself."""
    for n_pre_pad in range(1, down + 1):
        h = hfull[n_pre_pad:]
        half_len = (h.size - 1) // 2
        if h.size % 2 == 1 and down - half_len % down == n_pre_pad and (half_len + n_pre_pad) // down == n_pre_remove:
            assert not np.any(hfull[:n_pre_pad])
            return h.astype(np.float64) / up
    raise AssertionError("not scipy.signal.resample_poly's framing")


@pytest.mark.parametrize("up,down", SIX)
def test_ref64_is_scipy_resample_poly_with_the_same_taps(up, down):
    """<= 4e-15 absolute at n in {1, 2, tpp - 1, tpp, tpp + 1, 3 tpp + 5} on noise x 0.3, and sample by sample within scipy's own
    float64 error: scipy gets taps / up and multiplies by up again (two roundings, 2^-53 each, of every tap) and accumulates the at
    most tpp terms of an output one after the other in float64 (at most tpp - 1 roundings of partial sums below mag), so it may be
    off by (tpp + 2) 2^-53 mag, mag = sum |tap x| of the output; the reference itself is the correctly rounded sum (2^-53 |y|).
    That worst case is asserted sample by sample.  mag stays below 2 here (asserted), i.e. the absolute figure is 9 eps mag: it
    is what a sequential sum of a few hundred terms keeps when its rounding errors do not all point one way (measured: 1.2e-15
    at most), tighter than the worst case for the long filters, and seven orders below what one misplaced tap costs (the smallest
    tap, 2e-8, times a sample)."""
    import scipy.signal
    u, d, hfull, npr, tpp = G.product_filter(up, down)
    assert (u, d) == (up, down)
    window = _scipy_window(hfull, up, down, npr)
    worst, worst_rel = 0.0, 0.0
    for n in (1, 2, tpp - 1, tpp, tpp + 1, 3 * tpp + 5):
        x = G.signal("noise", n, n)
        y, mag = R.polyphase_ref64(x, up, down, hfull, npr, R.n_out_of(n, up, down))
        ref = scipy.signal.resample_poly(x.astype(np.float64), up, down, window=window)
        assert ref.shape == y.shape
        err = np.abs(ref - y)
        derived = (tpp + 2) * 2.0 ** -53 * mag + 2.0 ** -53 * np.abs(y)
        assert float(mag.max()) < 2.0
        assert np.all(err <= derived), (n, int(np.argmax(err > derived)))
        worst, worst_rel = max(worst, float(err.max())), max(worst_rel, float(np.max(err / np.maximum(derived, 1e-300))))
    print(f"{up}/{down} tpp {tpp}: reference vs scipy, worst {worst:.2e} absolute, {worst_rel:.3f} of scipy's own bound")
    assert worst <= 4e-15


def test_ref64_edges():
    """An empty tap range is +0.0; a zero-padded tap times NaN is NaN; infinities propagate with their sign; `outputs` selects."""
    hfull = np.float32([1.0, 2.0, 3.0, 4.0, 5.0])                     # up 3: rows [1, 4], [2, 5], [3, 0 (padding)]
    y, mag = R.polyphase_ref64(np.float32([1.0, -1.0]), 3, 2, hfull, 0, 8)
    # i = 0, 2, 4, 6, 8, 10, ..: (j0, p) = (0, 0), (0, 2), (1, 1), (2, 0), (2, 2), (3, 1), ..
    assert y.tolist() == [1.0, 3.0, -2.0 + 5.0, -4.0, 0.0, 0.0, 0.0, 0.0] and not np.any(np.signbit(y[4:]))   # m = 4 is 0 x -1
    assert mag.tolist() == [1.0, 3.0, 7.0, 4.0, 0.0, 0.0, 0.0, 0.0]
    assert R.tap_range(3, 2, 3, 2, 2, 0) == (2, 0, 1, 1) and R.tap_range(5, 2, 3, 2, 2, 0) == (3, 1, 2, 1)
    y, _ = R.polyphase_ref64(np.float32([np.nan, 1.0]), 3, 2, hfull, 0, 5)
    assert np.isnan(y).tolist() == [True, True, True, False, False]    # m = 1 meets NaN only through the tap 3; m = 2 through 5
    for first, want in ((7.0, 3.0), (np.nan, np.nan), (np.inf, np.nan)):  # i = 5: j0 = 1, row 2 = [3, 0]: 3 x 1 + 0 x first
        y, _ = R.polyphase_ref64(np.float32([first, 1.0]), 3, 1, hfull, 0, 6)
        assert y[5] == want or (np.isnan(want) and np.isnan(y[5]))
    y, _ = R.polyphase_ref64(np.float32([np.inf, -1.0]), 3, 2, -hfull, 0, 4)
    assert y.tolist() == [-np.inf, -np.inf, -np.inf, 4.0]                # m = 2 is -2 x -1 + -5 x Inf
    full, _ = R.polyphase_ref64(np.float32([1.0, -1.0]), 3, 2, hfull, 0, 8)
    part, _ = R.polyphase_ref64(np.float32([1.0, -1.0]), 3, 2, hfull, 0, 8, outputs=[2, 3])
    assert part.tolist() == [0.0, 0.0, full[2], full[3], 0.0, 0.0, 0.0, 0.0]


def test_assert_same_taps_is_half_an_ulp():
    """The bound at work: float32(y64) passes, the neighbouring float32 does not; ulp32 at the binade edges and at the floor."""
    assert R.ulp32(np.array([1.0, 1.5, 2.0 - 2.0 ** -30, 2.0, 0.75, 2.0 ** -126, 2.0 ** -127, 0.0])).tolist() == \
        [2.0 ** -23, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]
    y = np.array([0.1, -3.3, 1.0 - 2.0 ** -30, 0.0, np.nan, np.inf])
    mag = np.abs(y)
    ok = y.astype(np.float32)
    worst, differ = R.assert_same_taps(ok, y, mag, 528, "exact")
    assert worst <= 1.0 and differ == 0
    for k in range(3):
        off = ok.copy()
        off[k] = np.nextafter(off[k], np.float32(np.inf if ok[k] < y[k] else -np.inf))     # the neighbour on the far side of y
        with pytest.raises(AssertionError, match=f"output {k}"):
            R.assert_same_taps(off, y, mag, 528, "one ulp off")
    nan_moved = ok.copy(); nan_moved[3] = np.nan
    with pytest.raises(AssertionError, match="NaN set"):
        R.assert_same_taps(nan_moved, y, mag, 528, "NaN")
    with pytest.raises(AssertionError, match="infinities"):
        R.assert_same_taps(np.where(np.isinf(ok), -ok, ok), y, mag, 528, "Inf")


@pytest.mark.parametrize("up,down", G.PRODUCT_RATIOS)
def test_impulse_train_reads_every_tap_once(up, down):
    u, d, hfull, npr, tpp = G.product_filter(up, down)
    x, expected, idx = R.impulse_train(u, d, hfull, npr)
    hpad, _ = R.padded_taps(hfull, u)
    q = np.flatnonzero(x)
    assert q.size == d and np.all(x[q] == 1.0) and np.all(np.diff(q) == q[0]) and q[0] >= tpp + 1 and math.gcd(int(q[0]), d) == 1
    assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(tpp * u))           # every index of the padded filter, exactly once
    assert np.array_equal(expected[idx >= 0], hpad[idx[idx >= 0]]) and not np.any(expected[idx < 0])
    # the builder's answer is the reference's: the first and last outputs, every output behind a row's last tap, and a sample between
    rng = np.random.default_rng(0)
    last_taps = np.flatnonzero(idx >= (tpp - 1) * u)
    pick = np.unique(np.concatenate([np.arange(600), np.arange(expected.size - 600, expected.size), last_taps,
                                     rng.integers(0, expected.size, 1500)]))
    y, _ = R.polyphase_ref64(x, u, d, hfull, npr, expected.size, outputs=pick)
    assert np.array_equal(y[pick], expected[pick].astype(np.float64))
    print(f"impulse train {up}/{down}: {x.size} samples, spacing {int(q[0])}, {expected.size} outputs, {tpp * u} taps read once")


def _mutant_rejections(mutant, stop_at_first=True):
    """The cases of the GPU table on which `mutant` (rounded to float32, as a kernel would) fails assert_same_taps."""
    hits = []
    for up, down, n, name in G.cases():
        _, _, _, _, tpp = G.product_filter(up, down)
        _, y, mag = G.reference(up, down, n, name)
        _, y_mut, _ = G.reference(up, down, n, name, mutant)
        with np.errstate(over="ignore"):
            got = y_mut.astype(np.float32)
        try:
            R.assert_same_taps(got, y, mag, tpp, quiet=True)
        except AssertionError:
            hits.append((up, down, n, name))
            if stop_at_first:
                break
    return hits


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_rejected_on_the_gpu_case_table(mutant):
    """The three restated off-by-one errors - the last tap of every row dropped, the upper-sample clamp one too high, the output
    grid one step late - do not pass the comparisons of test_resample_pcm_edges_gpu.py: a kernel with one of them fails there."""
    hits = _mutant_rejections(mutant)
    print(f"{mutant}: rejected by assert_same_taps first on {hits[:1]}")
    assert hits
    # and the unmutated reference passes its own table (the comparisons are not simply always failing)
    up, down, n, name = hits[0]
    _, y, mag = G.reference(up, down, n, name)
    assert R.assert_same_taps(y.astype(np.float32), y, mag, G.product_filter(up, down)[4], quiet=True)[1] == 0


def test_the_dropped_last_tap_is_seen_where_it_is_small():
    """The mutant that today's 2e-6 cannot see, at the places built for it: on the product filters' long noise and edge-weighted
    cases (the ends of the rows are 2e-8 .. 7e-8) and, exactly, on the impulse train."""
    mutant = "t_hi_drops_last_tap"
    for up, down in G.PRODUCT_RATIOS:
        u, d, hfull, npr, tpp = G.product_filter(up, down)
        for name in ("noise", "edge"):
            _, y, mag = G.reference(up, down, 3 * tpp + 5, name)
            _, y_mut, _ = G.reference(up, down, 3 * tpp + 5, name, mutant)
            changed = float(np.max(np.abs(y_mut - y)))
            assert 0 < changed < 2e-6 * 0.3, changed                   # far inside the oracle tolerance ..
            with pytest.raises(AssertionError):                        # .. and outside the same-taps bound
                R.assert_same_taps(y_mut.astype(np.float32), y, mag, tpp, quiet=True)
        x, expected, idx = R.impulse_train(u, d, hfull, npr)
        behind_last = np.flatnonzero((idx >= (tpp - 1) * u) & (expected != 0))
        assert behind_last.size > 0
        y_mut, _ = R.polyphase_ref64(x, u, d, hfull, npr, expected.size, mutant=mutant, outputs=behind_last)
        assert np.all(y_mut[behind_last] == 0.0) and np.all(y_mut[behind_last].astype(np.float32) != expected[behind_last])


def test_pcm_known_answers_are_the_host_conversion():
    """The hand-derived words of the GPU tests against pcm_bytes_host, so that a slip in the table shows without a GPU."""
    v16, w16 = G.kat_arrays(G.PCM16_KAT)
    assert np.array_equal(pcm_bytes_host(v16, "PCM_16")[0].view("<i2"), w16)
    v24, w24 = G.kat_arrays(G.PCM24_KAT)
    assert v24.size == 27 and np.array_equal(pcm_bytes_host(v24, "PCM_24")[0], G.pcm24_bytes(w24))
    assert G.pcm24_bytes([-1, 1, -8388608]).tolist() == [255, 255, 255, 1, 0, 0, 0, 0, 128]
    # the ties are ties and the denormals are denormals in float32
    t16 = v16.astype(np.float64)[15:21] * 2.0 ** 31
    assert t16.tolist() == [65535.5, 65534.5, -65535.5, -65536.5, 0.5, -0.5]
    t24 = v24.astype(np.float64)[21:27] * 2.0 ** 31
    assert t24.tolist() == [255.5, 254.5, -255.5, -256.5, 0.5, -0.5]
    assert 0 < abs(float(v16[11])) < 2.0 ** -126 and v16[12] == -v16[11] and np.signbit(v16[1]) and np.signbit(v24[15])
