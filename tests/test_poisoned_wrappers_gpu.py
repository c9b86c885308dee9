"""Every kernel-launching wrapper of `_native.Context` under poisoned allocations (tests/poison_alloc.py): each entry of CALLS runs
unpoisoned, with every `torch.empty` of the wrapper filled with 0xFF and with 0x7F between 4 KiB guard bands, its device inputs
uploaded into guarded memory too, and the three results must be bit-identical and every guard intact.  That catches an output
element the kernel never writes, a kernel that accumulates into memory it assumes clear, a read outside an input that reaches a
result, and a store up to 4 KiB outside an allocation - whatever the values are, so no reference is needed here (the per-kernel
parity modules hold the references).

Shapes are the smallest that leave a ragged remainder in the kernel's loops (k * tile + 1 or a prime, two workgroups or more, an
empty and a one-element range where ranges are taken); where an edge-case module names such shapes they come from there.

What is compared is what the wrapper documents as its result.  Documented exemptions, each sliced in its `build`:
  pyin_viterbi   ptr[0]   "ptr [frames, 2 * n_bins] int16 holding uint16 back-pointers; row 0 is never written"
Buffers handed in as `out=` come from `upload` with a known filling and are compared WHOLE: the bytes behind `n_bytes`
(`pack_pcm_device`: "bytes behind them keep their values") and the row tails of a wide planar `out` (`decode_pcm`: "of which only the
first n_frames elements are written") must keep that filling.

The completeness check at the end runs without a GPU: a public method of Context is a key of CALLS or listed in NOT_KERNELS."""
import inspect

import numpy as np
import pytest
import torch

import poison_alloc as PA
from audio_cut_amd import _native

SR = 44100
CALLS = []              # (name, build): build(hip, upload) -> a zero-argument callable that makes the call and returns the outputs


def entry(name):
    def register(f):
        index = len(CALLS)
        CALLS.append((name, lambda hip, upload: f(hip, upload, np.random.default_rng(index))))
        return f
    return register


def method_of(name: str) -> str:
    return name.split("[")[0]


def _noise(rng, n, amp=0.3):
    return (amp * rng.standard_normal(n)).astype(np.float32)


def _segments(n):
    """(start, end) with an empty range at either end and inside, one-element ranges, the whole signal, ragged long ones."""
    s = [(0, 0), (3, 4), (0, n), (n, n), (n - 1, n), (100, 100 + 4097), (5000, 5000), (n // 2, n // 2 + 16 * 256 + 1)]
    return np.array([a for a, _ in s], np.int64), np.array([b for _, b in s], np.int64)


def _bars(nf):
    """(lo, hi) frame ranges: empty (hi == lo, hi < lo), one element, all frames, the last frame, ragged."""
    b = [(5, 5), (7, 3), (9, 10), (0, nf), (nf, nf), (nf - 1, nf), (0, 1), (11, 11 + 257), (nf // 2, nf // 2 + 64)]
    return np.array([a for a, _ in b], np.int64), np.array([h for _, h in b], np.int64)


# ---- framewise ------------------------------------------------------------------------------------------------------------------------
@entry("frame_rms")
def _(hip, upload, rng):
    import test_frame_features_edges_gpu as FE                      # RMS_CONFIGS and the length with one frame in the last block
    cfgs = [c for c in FE.RMS_CONFIGS if c in ((7, 3), (2205, 882), (8192, 441), (15360, 5000))]
    xs = {(f, h, c): upload(_noise(rng, FE._rms_lengths(f, h, c)[-1])) for f, h in cfgs for c in (True, False)}
    return lambda: {str(k): hip.frame_rms(x, k[0], k[1], center=k[2]) for k, x in xs.items()}


@entry("frame_rms_multi")
def _(hip, upload, rng):
    x1, x2 = upload(_noise(rng, 8193)), upload(_noise(rng, 5 * 8192 + 1))        # test_frame_rms_multi_edges: 8193; then several blocks
    cfgs = [(2205, 882), (1411, 1411), (441, 2000), (8191, 4096)]
    return lambda: [hip.frame_rms_multi(x1, cfgs), hip.frame_rms_multi(x2, cfgs), hip.frame_rms_multi(x2, cfgs[:1])]


def _stft_x(rng, upload):
    return upload(_noise(rng, 5 * 2048 + 1))                        # STFT_LENGTHS ends at 2049: one past a frame; here 24 frames at hop 441


@entry("stft2048_features")
def _(hip, upload, rng):
    x = _stft_x(rng, upload)
    n = 5000                                                        # test_stft2048_grouped_windows_cut_by_their_bounds
    frames = [(2500, 2400, 2600), (2500, 2500, 2501), (2500, 2500, 2500), (2500, 0, 0), (-1024, 0, n), (-4000, 0, n), (n + 1023, 0, n),
              (n + 9000, 0, n), (0, 0, n), (n, 0, n), (1024, 1, 2047)]
    xg = upload(_noise(rng, n))
    fc, lo, hi = (upload(np.array([fr[k] for fr in frames], dtype=np.int64)) for k in range(3))
    return lambda: [hip.stft2048_features(x, 441, want_flat=True, want_mel=True), hip.stft2048_features(x, 4096, want_flat=False, want_mel=True),
                    hip.stft2048_features(xg, 441, want_flat=True, want_mel=True, frame_center=fc, frame_lo=lo, frame_hi=hi)]


@entry("stft2048_flatness")
def _(hip, upload, rng):
    x = _stft_x(rng, upload)
    return lambda: hip.stft2048_flatness(x, 512)


@entry("onset_strength")
def _(hip, upload, rng):
    import frame_refs as R
    import test_frame_features_edges_gpu as FE
    hop = 441
    pad = R.onset_pad(hop)
    lengths = [1, 2, pad, pad + 1, pad + 2, 23]                     # _onset_pool's lengths, one group each
    mel = upload(np.concatenate([FE._onset_group(("wide", "quiet", "zeros", "ties", "flat", "wide")[i], n, rng) for i, n in enumerate(lengths)]))
    gs = np.concatenate(([0], np.cumsum(lengths))).tolist()
    return lambda: [hip.onset_strength(mel, hop, "mean", gs), hip.onset_strength(mel, hop, "median", gs), hip.onset_strength(mel, hop)]


@entry("tempogram_reduce")
def _(hip, upload, rng):
    import test_frame_features_edges_gpu as FE
    cases = [(win, n, upload(FE._tg_envelopes(n, int(rng.integers(1 << 30)))["dense"]), FE._tg_logprior(win))
             for win, n in ((160, 130), (689, 695), (1024, 65), (3, 1))]          # TG_WINS x _tg_lengths: n > win, n < win // 2, one frame
    return lambda: [hip.tempogram_reduce(env, win, lp, want_argmax=bool(k % 2 == 0)) for k, (win, n, env, lp) in enumerate(cases)]


@entry("yin_f0")
def _(hip, upload, rng):
    import test_frame_features_edges_gpu as FE
    sr, fmin, fmax = FE.YIN_RANGES["music"]
    x = upload(_noise(rng, FE._yin_lengths(2048)[-1]))              # 3 * 2048 + 17
    p = FE.YIN_PLATEAU
    xp = upload(FE._yin_plateau_signals()["impulses_22"])
    return lambda: [hip.yin_f0(x, sr, fmin, fmax, 2048, 512, want_cmnd=True), hip.yin_f0(x, sr, fmin, fmax, 2048, 441),
                    hip.yin_f0(xp, p["sr"], p["fmin"], p["fmax"], p["frame_length"], p["hop"], p["threshold"], want_cmnd=True)]


# ---- resamplers, Silero, PCM in and out ---------------------------------------------------------------------------------------------
def _resample_cases(rng, upload):
    import test_resample_pcm_edges_gpu as RE
    return [(up, down, upload(_noise(rng, n))) for up, down in RE.RATIOS for n in RE.case_lengths(up, down)[5:]]    # 3 tpp + 5 and the counts 0, 1, 31 mod 32


@entry("resample_poly")
def _(hip, upload, rng):
    cases = _resample_cases(rng, upload)
    return lambda: [hip.resample_poly(x, up, down) for up, down, x in cases]


@entry("resample_poly_pcm16")
def _(hip, upload, rng):
    cases = _resample_cases(rng, upload)
    return lambda: [hip.resample_poly_pcm16(x, up, down) for up, down, x in cases]


@entry("resample_poly_segments")
def _(hip, upload, rng):
    lens = [11289, 0, 1, 9000, 200, 1]                              # test_precompute_chain's chunks, an empty and two one-sample segments
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1].tolist()
    x = upload(_noise(rng, sum(lens)))
    return lambda: [hip.resample_poly_segments(x, offs, lens, up, down, bucket=b) for up, down in ((160, 441), (147, 160)) for b in (0, 1000, 4096)]


@entry("silero_probs")
def _(hip, upload, rng):
    import test_silero_kernels_gpu as TS
    _, dev = TS.packed(hip, 1)
    p = {k: upload(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v for k, v in dev.items()}
    counts = [1, 0, 5, 1, 10]                                       # test_lstm_chunk_layout's layout with 17 windows: two front-end workgroups + 1
    firsts = [0, 1, 1, 6, 7]
    ws = sum((TS.one_chunk(c, base=512 * f) for f, c in zip(firsts, counts) if c), [])
    x16 = upload(_noise(rng, 512 * sum(counts)))
    return lambda: hip.silero_probs(x16, np.array(ws, np.int64), np.array(firsts, np.int32), np.array(counts, np.int32), p)


PACK_NS = (1, 5, 1025, 4099)                                        # FRAMES of test_wav_decode_gpu.py: below a quad, a workgroup + 1, several + 3


@entry("pack_pcm24")
def _(hip, upload, rng):
    xs = [upload(_noise(rng, n, 0.5)) for n in PACK_NS]
    return lambda: [hip.pack_pcm24(x) for x in xs]


@entry("pack_pcm_device")
def _(hip, upload, rng):
    mono = [upload(_noise(rng, n, 0.5)) for n in PACK_NS]
    wide = [upload(_noise(rng, (2, n + 5), 0.5))[:, :n] for n in PACK_NS]      # rows that are views into wider rows
    spare = 64

    def call():
        res = {}
        for sub, (_, width) in _native.PACK_SUBTYPES.items():
            for x in mono + wide:
                key = f"{sub}/{tuple(x.shape)}"
                res[key] = hip.pack_pcm_device(x, sub)
                # "`out`: a uint8 device tensor of at least that many bytes to write into; bytes behind them keep their values": the
                # whole buffer is compared, the spare bytes must still hold 0xA5
                out = upload(np.full(x.numel() * width + spare, 0xA5, np.uint8))
                res[key + "/out="] = (hip.pack_pcm_device(x, sub, out=out), out)
        return res
    return call


@entry("pack_pcm")
def _(hip, upload, rng):
    x, st = upload(_noise(rng, 4099, 0.5)), upload(_noise(rng, (2, 1025), 0.5))
    return lambda: [hip.pack_pcm(x, "PCM_16"), hip.pack_pcm(st, "FLOAT")]


@entry("decode_pcm")
def _(hip, upload, rng):
    import test_wav_decode_gpu as WD
    from audio_cut_amd.utils import wav_reader as WR
    cases = []
    for fmt in WD.FORMATS:
        for channels in (1, 2, 3):
            for n in (5, 1025, 4099):                               # of WD.FRAMES: a quad + 1, a pass + 1, several workgroups + 3
                cases.append((WD._info(fmt, channels, n), upload(WD._random_bytes(rng, fmt, n * channels))))

    def call():
        res = []
        for info, raw in cases:
            n, ch = info.n_frames, info.channels
            res.append((hip.decode_pcm(raw, info, WR.LAYOUT_MONO), hip.decode_pcm(raw, info, WR.LAYOUT_PLANAR)))
            # "the rows of a given `out` [channels, stride >= n_frames], of which only the first n_frames elements are written": the
            # whole wide buffer is compared, the row tails must still hold the canary
            wide = upload(np.full((ch, n + 5), WD.CANARY, np.float32))
            flat = upload(np.full(n, WD.CANARY, np.float32))
            res.append((hip.decode_pcm(raw, info, WR.LAYOUT_PLANAR, out=wide), hip.decode_pcm(raw, info, WR.LAYOUT_MONO, out=flat)))
        return res
    return call


# ---- boundary policy, bars, gates ------------------------------------------------------------------------------------------------------
N_SEG = 40961                                                       # 10 * 4096 + 1


@entry("segment_frame_rms")
def _(hip, upload, rng):
    x = upload(_noise(rng, N_SEG))
    a, b = _segments(N_SEG)
    return lambda: [hip.segment_frame_rms(x, a, b, 2205, 882, center=True), hip.segment_frame_rms(x, a, b, 2205, 882, center=False),
                    hip.segment_frame_rms(x, a, b, 7, 3, center=True)]


@entry("segment_sumsq_peak")
def _(hip, upload, rng):
    x = upload(_noise(rng, N_SEG))
    a, b = _segments(N_SEG)
    return lambda: [hip.segment_sumsq_peak(x, a, b), hip.segment_sumsq_peak(x, a[:1], b[:1])]


@entry("bar_energy_silence")
def _(hip, upload, rng):
    nf = 1025
    rms = upload(np.abs(_noise(rng, nf, 0.05)))
    lo, hi = _bars(nf)
    return lambda: [hip.bar_energy_silence(rms, lo, hi, -30.0), hip.bar_energy_silence(rms, lo[:1], hi[:1], -30.0)]


@entry("segment_pair_energy")
def _(hip, upload, rng):
    v, i = upload(_noise(rng, N_SEG)), upload(_noise(rng, N_SEG))
    a, b = _segments(N_SEG)
    return lambda: [hip.segment_pair_energy(v, i, a, b), hip.segment_pair_energy(v, None, a, b)]


@entry("stft2048_centroid_bandwidth")
def _(hip, upload, rng):
    x = _stft_x(rng, upload)
    return lambda: [hip.stft2048_centroid_bandwidth(x, SR, 512), hip.stft2048_centroid_bandwidth(x, SR, 4096)]


@entry("bar_means3")
def _(hip, upload, rng):
    nf = 1025
    rms = upload(np.abs(_noise(rng, nf, 0.05)))
    cen, bw = upload(2000.0 + 500.0 * rng.standard_normal(nf)), upload(1500.0 + 300.0 * rng.standard_normal(nf))
    lo, hi = _bars(nf)
    return lambda: [hip.bar_means3(rms, cen, bw, lo, hi), hip.bar_means3(rms, cen, bw, lo[:2], hi[:2])]


@entry("quiet_gate")
def _(hip, upload, rng):
    hw = 441                                                        # test_quiet_gate_meansq_against_numpy's edge centres
    n = 5 * hw + 1
    x = upload(_noise(rng, n, 0.2))
    edge = [-hw - 1, -hw, -1, 0, hw, n - 1, n, n + hw - 1, n + hw, n + hw + 1, 3 * hw, 10 ** 12, -10 ** 12]
    centers = np.array(edge + rng.integers(-2 * hw, n + 2 * hw, size=300).tolist(), dtype=np.int64)
    return lambda: [hip.quiet_gate(x, hw, centers), hip.quiet_gate(x, hw, []), hip.quiet_gate(x, 1, centers[:1])]


@entry("vocal_coverage")
def _(hip, upload, rng):
    x = upload(_noise(rng, 4 * 256 * 3 + 2))                        # three workgroups' quads and a tail; the slice starts 4 bytes off 8-byte alignment
    return lambda: [hip.vocal_coverage(x), hip.vocal_coverage(x[1:]), hip.vocal_coverage(x[:1]), hip.vocal_coverage(x, rel=0.5, abs_floor=0.1)]


@entry("local_valley")
def _(hip, upload, rng):
    n = 40001
    x = upload(_noise(rng, n))
    centers = np.array([0, 20000, n, 1500, n - 100, 1], np.int64)  # clipped at either end (tests/test_kernels_edges_gpu.py::_check_valley)
    return lambda: [hip.local_valley(x, centers, 3000, 441), hip.local_valley(x, centers, 3000, 1), hip.local_valley(x, centers[:1], 300, 2048)]


# ---- pitch ---------------------------------------------------------------------------------------------------------------------------------
@entry("pyin_observe")
def _(hip, upload, rng):
    import test_pitch_kernels_gpu as TP                             # its cached crafted launches (OBSERVE_IDS)
    ls = [TP._launches()[name] for name in ("crafted", "lags3", "lags1023", "bins1")]
    rows = [upload(np.ascontiguousarray(l["rows"], dtype=np.float64)) for l in ls]
    return lambda: [hip.pyin_observe(r, l["sr"], l["fmin"], l["min_period"], l["n_bins"], l["bps"]) for r, l in zip(rows, ls)]


@entry("pyin_viterbi")
def _(hip, upload, rng):
    import pitch_refs as P
    cases = []
    for name in ("bins31", "bins513", "one_frame", "two_frames", "ties_two_passes"):
        _, kind, n_bins, half, n_frames, seed = next(c for c in P.VITERBI_CASES if c[0] == name)
        c = P.viterbi_case(kind, n_bins, half, n_frames, seed, P.VITERBI_PLANTS.get(name, ()))
        cases.append((c, upload(c["logv"]), upload(c["logu"])))

    def call():
        res = []
        for c, logv, logu in cases:
            states, ptr = hip.pyin_viterbi(logv, logu, c["n_bins"], c["half"], c["lt_same"], c["lt_cross"], c["lt_zero"], c["log_p_init"])
            # "ptr [frames, 2 * n_bins] int16 holding uint16 back-pointers; row 0 is never written"
            res.append((states, ptr[1:]))
        return res
    return call


@entry("lpc_formants")
def _(hip, upload, rng):
    import test_pitch_kernels_gpu as TP                             # its cached cases (LPC_IDS)
    cs = [TP._lpc_cases()[name] for name in ("len4_order1", "len257", "hop_divides_plus_1", "zero_frames", "len2048_order32")]
    xs = [upload(np.ascontiguousarray(c["x"], dtype=np.float32)) for c in cs]
    return lambda: [hip.lpc_formants(x, c["frame_len"], c["hop"], order=c["order"], preemph=c["preemph"]) for x, c in zip(xs, cs)]


@entry("zero_crossing_rate")
def _(hip, upload, rng):
    x = _stft_x(rng, upload)
    return lambda: [hip.zero_crossing_rate(x, 2048, 512), hip.zero_crossing_rate(x, 2047, 441), hip.zero_crossing_rate(x[:1], 2048, 512)]


@entry("stft2048_spectral")
def _(hip, upload, rng):
    x = _stft_x(rng, upload)
    return lambda: [hip.stft2048_spectral(x, SR, 512), hip.stft2048_spectral(x[:1], SR, 441)]


# ---- cut-point refinement (the sizes of tests/test_cut_refine_edges_gpu.py) -----------------------------------------------------------
@entry("moving_meansq_db")
def _(hip, upload, rng):
    x = upload(_noise(rng, 2 * 8192 + 1))
    short = upload(_noise(rng, 300))
    return lambda: [hip.moving_meansq_db(x, w) for w in (1, 257, 3528, 8192)] + [hip.moving_meansq_db(short, 441)]


@entry("next_leq_scan")
def _(hip, upload, rng):
    dbs = []
    for n in (1, 4095, 4097, 257 * 4096 + 1):                       # one block -+ 1, and 258 blocks: carry threads that own two
        db = np.ones(n)
        db[rng.random(n) < 0.001] = -1.0
        db[-1] = 1.0
        dbs.append(upload(db))
    return lambda: [hip.next_leq_scan(db, 0.0) for db in dbs]


@entry("window_argmin")
def _(hip, upload, rng):
    n = 50_000
    db = upload(np.repeat(np.round(rng.uniform(-80.0, -20.0, n // 8), 0), 8))
    starts, lens = [], []
    for ln in (1, 2, 255, 256, 257, 19845):
        for s in (0, 1, 255, n - 1, n - ln, n - ln // 2 - 1):
            starts.append(s); lens.append(ln)
    s, ln = np.array(starts + [0], np.int64), np.array(lens + [n + 5], np.int64)
    return lambda: [hip.window_argmin(db, s, ln), hip.window_argmin(db, s[:1], ln[:1])]


@entry("zero_cross_nearest")
def _(hip, upload, rng):
    n = 20_001
    x = _noise(rng, n)
    x[:8000] = 0.25 + np.abs(x[:8000])                              # a stretch without any crossing: NaN results
    x[0] = x[-1] = 0.0
    xd = upload(x)
    idx = np.array([1, 2, 65, 66, 4000, 7999, 8000, n - 66, n - 2, n - 1] + rng.integers(1, n - 1, 200).tolist(), np.int64)
    return lambda: [hip.zero_cross_nearest(xd, idx, half) for half in (1, 63, 64, 65, 353)]


@entry("quiet_guard_slow")
def _(hip, upload, rng):
    def case(span, win):                                            # test_quiet_guard_slow_edges, two of its (span, win) pairs
        n = 6 * span + 3 * win
        x = _noise(rng, n, 0.05)
        x[2 * span: 2 * span + span // 2] = 0.0
        x[n - win // 3:] = np.abs(x[n - win // 3:])
        idx = np.array([0, 1, -3, 255, 2 * span + 5, n - span, n - win - 1, n - win, n - win + 1, n - 3, n - 2, n - 1]
                       + rng.integers(0, n - 1, 20).tolist(), np.int64)
        return upload(x), idx, span, win
    cases = [case(6615, 441), case(300, 7), case(6615, 7)]
    return lambda: [hip.quiet_guard_slow(*c) for c in cases]


@entry("pause_cut_points")
def _(hip, upload, rng):
    n = 6 * 4096 * 4 + 1
    x = _noise(rng, n, 0.1)
    x[30_000: 30_300] = 0.0

    def case(win, guard):
        a = [0, 10_000, 70_000, 80_000, 80_100, 80_200, 80_300, n - 3, n - 40_000, 500]
        m = [6000, 4 * 4096 + 4097, 2, win - 1, win, win + 1, 1, 3, 40_000, 0]   # 2, win -+ 1, m <= 1 (cut -1), pauses that end at n
        return np.array(a, np.int64), np.array(a, np.int64) + np.array(m, np.int64), win, guard
    xd = upload(x)
    cases = [case(1102, 5292), case(7, 64), case(1102, 0)]
    return lambda: [hip.pause_cut_points(xd, *c) for c in cases]


# ---- MDX23 front and back end (plans of tests/test_mdx_kernels_gpu.py) ---------------------------------------------------------------
def _mdx_stft(stereo):
    def build(hip, upload, rng):
        import mdx_refs as R
        chunks = [(0, 1), (200, R.GEN + 1)]                         # CHUNK_LENGTHS' ends: one sample; GEN + 1 = two items, the second nearly all padding
        track = upload(_noise(rng, (2, R.GEN + 300) if stereo else R.GEN + 300))
        cs, cl, wi = (upload(t) for t in R.item_tables([(a, a + n, a, a + n) for a, n in chunks]))
        one = [upload(t) for t in R.item_tables([(100, 100 + 4095, 100, 100 + 4095)])]

        def call():
            amax = torch.zeros((cs.numel(), R.T), dtype=torch.float32, device=hip.device)       # "zeroed by the caller", as the backend does
            out = upload(np.full((1, 4, R.T, R.F), 7.0, np.float32))
            return [hip.mdx_stft(track, cs, cl, wi, amax=amax), amax, hip.mdx_stft(track, cs[:1], cl[:1], wi[:1]),
                    hip.mdx_stft(track, *one, out=out)]
        return call
    return build


entry("mdx_stft[mono]")(_mdx_stft(False))
entry("mdx_stft[stereo]")(_mdx_stft(True))


@entry("mdx_istft")
def _(hip, upload, rng):
    import mdx_refs as R
    spec = upload(rng.standard_normal((2, 4, R.T, R.F), dtype=np.float32))
    return lambda: [hip.mdx_istft(spec), hip.mdx_istft(spec[1:])]


def _mdx_plan(key, stereo, rng, upload):
    import mdx_refs as R
    from test_mdx_kernels_gpu import OLA_BY_ID
    _, n, args = OLA_BY_ID[key][:3]
    ranges = R.plan_ranges(n, **args)
    n_items = len(R.item_tables(ranges)[0])
    track = upload(_noise(rng, (2, n) if stereo else n))
    wave = upload(0.3 * rng.standard_normal((n_items, 2, R.ITEM), dtype=np.float32))
    return [track, wave] + [upload(t) for t in R.chunk_tables(ranges)]


def _mdx_ola(stereo):
    def build(hip, upload, rng):
        plans = [_mdx_plan(k, stereo, rng, upload) for k in ("empty_regions", "257_samples", "one_sample")]     # gaps no region covers; tiny tracks
        return lambda: [hip.mdx_assemble_ola(*p) for p in plans] + ([hip.mdx_assemble_ola(*plans[1], stereo_stems=False)] if stereo else [])
    return build


entry("mdx_assemble_ola[mono]")(_mdx_ola(False))
entry("mdx_assemble_ola[stereo]")(_mdx_ola(True))


def _mdx_chunk_vocal(stereo):
    def build(hip, upload, rng):
        import mdx_refs as R
        lens = [1000, R.GEN + 1, 4095, 1]                           # tests/test_kernels_edges_gpu.py: one item, two items, one sample
        n_it = [len(R.item_tables([(0, cl, 0, cl)])[0]) for cl in lens]
        base = np.concatenate(([0], np.cumsum(n_it)[:-1])).astype(np.int32)
        offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        total = int(offsets[-1])
        track = upload(_noise(rng, (2, total) if stereo else total))
        wave = upload(0.3 * rng.standard_normal((sum(n_it), 2, R.ITEM), dtype=np.float32))
        args = (track, wave, upload(offsets[:-1].copy()), upload(np.asarray(lens, np.int64)), upload(offsets[:-1].copy()), upload(base), total)
        return lambda: [hip.mdx_chunk_vocal(*args)] + ([hip.mdx_chunk_vocal(*args, mix_minus=True)] if stereo else [])
    return build


entry("mdx_chunk_vocal[mono]")(_mdx_chunk_vocal(False))
entry("mdx_chunk_vocal[stereo]")(_mdx_chunk_vocal(True))


def _mdx_pcm(stereo, subtype):
    def build(hip, upload, rng):
        plans = [_mdx_plan(k, stereo, rng, upload) for k in ("empty_regions", "257_samples", "one_sample")]
        return lambda: [hip.mdx_assemble_pcm(*p, subtype) for p in plans]
    return build


for _stereo in (False, True):
    for _sub in ("PCM_24", "DOUBLE"):
        entry(f"mdx_assemble_pcm[{'stereo' if _stereo else 'mono'}-{_sub}]")(_mdx_pcm(_stereo, _sub))


@entry("mdx_assemble_pcm24")
def _(hip, upload, rng):
    plan = _mdx_plan("257_samples", True, rng, upload)
    return lambda: hip.mdx_assemble_pcm24(*plan)


# ---- U-Net layers (unet_exact.CASES through run_case: per kind the one-tile case and the swizzled / several-workgroup one) ----------------
def _unet(case_ids, takes_out=False):
    def build(hip, upload, rng):
        import unet_exact as UE
        from test_unet_kernel_envelope_gpu import KIND, TAKES_AMAX, run_case

        def call():
            res = {}
            for cid in case_ids:
                case = UE.case_of(cid, "gauss")
                y = res[cid] = run_case(hip, case, upload=upload)
                if takes_out:
                    res[cid + "/out="] = run_case(hip, case, upload=upload, out=upload(np.full(tuple(y.shape), 7.0, np.float32)))
                if TAKES_AMAX[cid]:
                    oa = torch.zeros((y.shape[0], y.shape[2]), dtype=torch.float32, device=hip.device)      # as the product does
                    if KIND[cid] in UE.SPLIT_KINDS:
                        lv = UE.case_of(cid, "xlo", levels=True)
                        res[cid + "/amax"] = (run_case(hip, lv, in_amax=lv.in_amax, out_amax=oa, upload=upload), oa)
                    else:
                        res[cid + "/amax"] = (run_case(hip, case, out_amax=oa, upload=upload), oa)
            return res
        return call
    return build


entry("conv3x3_f16x3")(_unet(("conv-one_tile-relu", "conv-16x64-B2-swizzle"), takes_out=True))
entry("conv3x3_f16x3_w96")(_unet(("conv_w96-one_tile-relu", "conv_w96-16x64-B2-swizzle"), takes_out=True))
entry("conv3x3_f16x3_s8")(_unet(("conv_s8-one_tile-relu", "conv_s8-16x64-B2-swizzle"), takes_out=True))
entry("conv3x3_f16x3_first")(_unet(("first-c0_4-ci48-one_tile", "first-c0_3-ci64-16x64-B2")))
entry("tdf_linear_f16x3")(_unet(("tdf-min-N96", "tdf-nblk8-supergroups", "tdf-T16-B2")))
entry("tdf_small_fused")(_unet(("tdf_small-F32-Hd5-M32", "tdf_small-B3-C8-T8-F96-Hd24", "tdf_small-B2-C3-T16-channel_mid_wave")))
entry("conv1x1_small")(_unet(("conv1x1-8to9-P4-B3-relu", "conv1x1-9to8-P4-B3-norelu")))
entry("down2x_f16x3")(_unet(("down-ci8-co8", "down-16x64-co104-swizzle")))
entry("up2x_f16x3")(_unet(("up-ci1-co24", "up-4x64-co48-swizzle")))


@entry("tdf_linear_final_f16x3")
def _(hip, upload, rng):
    import test_tdf_final_fused_gpu as TF
    cases = []
    for name in ("one_workgroup_one_stage", "t6_odd_stage_count", "three_output_channels"):
        shape, c_out, extra = TF.CASES[name]
        d = TF._case(torch.device("cpu"), *shape, c_out, seed=11 + len(name), **extra)
        cases.append({k: upload(v.numpy()) if isinstance(v, torch.Tensor) else v for k, v in d.items()})
    return lambda: [TF._fused(hip, d, want_y=w) for d in cases for w in (True, False)]


# ---- plain reductions ------------------------------------------------------------------------------------------------------------------
@entry("sum_squares_parts")
def _(hip, upload, rng):
    xs = [upload(_noise(rng, n)) for n in (1, 4095, 3 * 4096 + 1, 37 * 4096 + 1)]        # one part; three and 37 parts with a tail
    return lambda: [hip.sum_squares_parts(x) for x in xs]


@entry("window_mean_squares")
def _(hip, upload, rng):
    n = 3 * 8191 + 1
    x = upload(_noise(rng, n))
    starts = np.array([0, 17, n, n - 5, n - 8191, 0, 100], np.int64)
    lens = np.array([0, 0, 0, 5, 8191, 1, 4097], np.int64)
    return lambda: [hip.window_mean_squares(x, starts, starts + lens), hip.window_mean_squares(x, starts[:1], starts[:1])]


# ---------------------------------------------------------------------------------------------------------------------------------------
NOT_KERNELS = {
    "close": "destroys the handle",
    "to_device": "a copy: pinned staging and PyTorch's own upload",
    "prefetch_begin": "prefetch cache bookkeeping",
    "prefetch": "runs another wrapper (which has its own row) and keeps its result",
    "prefetch_stats": "prefetch cache bookkeeping",
    "prefetch_frame_rms_multi": "frame_rms_multi (which has its own row) stored in the prefetch cache",
    "pyin_transition_tables": "host tables (numpy / scipy), no launch",
    "tdf_final_tileable": "a shape predicate, no launch",
    "pyin": "composition of yin_f0, pyin_observe and pyin_viterbi with host arithmetic in between",
    "mean_square": "composition: sum_squares_parts and a host sum",
}
COMPOSITIONS = {"pyin": ("yin_f0", "pyin_observe", "pyin_viterbi"), "mean_square": ("sum_squares_parts",)}


@pytest.fixture
def run_three(hip_ctx):
    return lambda fn: PA.run_three(hip_ctx, fn)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CALLS])
def test_wrapper_is_independent_of_what_its_allocations_held(hip_ctx, run_three, name):
    build = dict(CALLS)[name]
    run_three(lambda upload: build(hip_ctx, upload)())


@pytest.mark.gpu
def test_the_harness_sees_planted_mistakes_on_the_device(hip_ctx):
    """What tests/test_poison_alloc_host.py shows on CPU tensors, once on the device: a wrapper's allocations are caught (the device
    filter matches the context's device), an unwritten element and a store past the end - into guard memory the test owns - are
    reported, and both functions are restored."""
    real = torch.empty
    x = _noise(np.random.default_rng(0), 4097)
    with PA.poisoned(0xFF) as pa:
        got = hip_ctx.frame_rms(PA.guarded_upload(hip_ctx, x), 441, 441)
        assert len(pa.registry) == 2 and got.data_ptr() == pa.registry[1][0].data_ptr() + PA.GUARD and not bool(torch.isnan(got).any())
        pa.check_guards()
        out = torch.empty(37, dtype=torch.float32, device=hip_ctx.device)
        assert bool(torch.isnan(out).all())
        torch.as_strided(out, (38,), (1,), storage_offset=out.storage_offset()).fill_(1.0)
        with pytest.raises(AssertionError, match=r"allocation #2 \(torch.float32, shape \(37,\), 148 bytes\).*offset 148 relative"):
            pa.check_guards()
    assert torch.empty is real

    def unwritten(upload):
        out = torch.empty(37, dtype=torch.float32, device=hip_ctx.device)
        out[:36] = upload(x[:36]) * 2
        return out
    with pytest.raises(AssertionError, match=r"result \(tensor torch.float32 \(37,\)\) differs .* first at byte 14[4-7] of 148"):
        PA.run_three(hip_ctx, unwritten)
    assert torch.empty is real


def test_every_public_method_has_a_row_or_a_reason():
    public = {n for n, m in inspect.getmembers(_native.Context, predicate=callable) if not n.startswith("_")}
    covered = {method_of(n) for n, _ in CALLS}
    assert len(dict(CALLS)) == len(CALLS), "two entries share a name"
    assert covered <= public, f"rows for methods that do not exist: {sorted(covered - public)}"
    assert not covered & set(NOT_KERNELS), sorted(covered & set(NOT_KERNELS))
    assert set(NOT_KERNELS) <= public, f"reasons for methods that do not exist: {sorted(set(NOT_KERNELS) - public)}"
    missing = public - covered - set(NOT_KERNELS)
    assert not missing, f"new wrappers without a row in CALLS (or a reason in NOT_KERNELS): {sorted(missing)}"
    for name, parts in COMPOSITIONS.items():
        assert name in NOT_KERNELS and set(parts) <= covered, name
    for form in ("mono", "stereo"):
        for m in ("mdx_stft", "mdx_assemble_ola", "mdx_chunk_vocal"):
            assert f"{m}[{form}]" in dict(CALLS)
        for sub in ("PCM_24", "DOUBLE"):
            assert f"mdx_assemble_pcm[{form}-{sub}]" in dict(CALLS)
