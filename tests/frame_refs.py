"""Plain float64 references of the framewise feature kernels (audio_cut_amd/csrc/ac_frames.hip), written from the definitions and
independent of the oracle's algorithms: explicit slices where the oracle strides, a direct autocorrelation where it goes through the
FFT, a per-frame loop where it works on matrices.  numpy only; tests/test_frame_features_edges_gpu.py pins them against
oracle.librosa_ops on the CPU and then holds the kernels to them at the edges."""
import numpy as np

N_FFT = 2048
F64_TINY = float(np.finfo(np.float64).tiny)
_MEL = {}


def rms_direct(x, frame, hop, center=True):
    """Framed RMS: zero padding of frame // 2 on both sides when centred, one explicit slice per frame, float64 sum of squares."""
    x = np.asarray(x, dtype=np.float64)
    pad = frame // 2 if center else 0
    xp = np.concatenate([np.zeros(pad), x, np.zeros(pad)])
    if len(xp) < frame:
        raise ValueError("signal shorter than one frame")
    nf = 1 + (len(xp) - frame) // hop
    out = np.empty(nf, dtype=np.float64)
    for f in range(nf):
        s = xp[f * hop: f * hop + frame]
        out[f] = np.sqrt(np.dot(s, s) / frame)
    return out


def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def mel_basis(sr):
    if sr not in _MEL:
        from oracle.librosa_ops import mel_filters
        _MEL[sr] = mel_filters(sr, N_FFT, n_mels=128, fmin=0.0, fmax=0.5 * sr).astype(np.float64)
    return _MEL[sr]


def stft_frame_direct(x, centre, lo=0, hi=None, sr=44100):
    """One 2048-sample frame centred on `centre`; samples outside [lo, hi) count as zero.  0 <= lo <= hi <= len(x) is the caller's
    duty, here as in ac_stft2048_features (which reads x[lo .. hi) unchecked: the bounds live in device arrays).
    float64 periodic Hann and rfft, rounded to complex64, magnitude and power in float32 (librosa's storage), then in float64:
    flatness = geometric / arithmetic mean of max(1e-10, power) over the 1025 bins, mel = basis @ power.
    Returns (flatness, mel[128], power[1025] float32)."""
    x = np.asarray(x)
    n = len(x)
    hi = n if hi is None else hi
    if not 0 <= lo <= hi <= n:
        raise ValueError("0 <= lo <= hi <= len(x)")
    fr = np.zeros(N_FFT, dtype=np.float64)
    for i in range(N_FFT):
        g = centre - N_FFT // 2 + i
        if lo <= g < hi:
            fr[i] = x[g]
    spec = np.fft.rfft(hann_periodic(N_FFT) * fr).astype(np.complex64)
    mag = np.abs(spec)
    power = mag * mag
    assert power.dtype == np.float32
    st = np.maximum(np.float32(1e-10), power).astype(np.float64)
    flat = np.exp(np.mean(np.log(st))) / np.mean(st)
    return float(flat), mel_basis(sr) @ power.astype(np.float64), power


def onset_pad(hop):
    return 1 + N_FFT // (2 * hop)


def onset_from_mel(mel, hop, aggregate="mean", group_start=None):
    """Onset strength of a mel power matrix [frames, 128], group by group: dB (amin 1e-10, clipped 80 dB under the group's own
    maximum), positive lag-1 difference, mean or median over the bands, `onset_pad(hop)` zeros in front, cut to the group length."""
    mel = np.asarray(mel, dtype=np.float64)
    nf = mel.shape[0]
    gs = [0, nf] if group_start is None else list(group_start)
    agg = {"mean": np.mean, "median": np.median}[aggregate]
    pad = onset_pad(hop)
    out = np.zeros(nf, dtype=np.float64)
    for a, b in zip(gs[:-1], gs[1:]):
        if b <= a:
            continue
        db = 10.0 * np.log10(np.maximum(1e-10, mel[a:b]))
        db = np.maximum(db, db.max() - 80.0)
        for t in range(b - a - 1):
            if pad + t < b - a:
                out[a + pad + t] = agg(np.maximum(0.0, db[t + 1] - db[t]))
    return out


def ramp_padded(env, p):
    """np.pad(env, (p, p), mode="linear_ramp", end_values=0) of a float32 series, written out: each ramp is
    k * (edge / p) for k = 0 .. p - 1 in float64, stored as float32, rising to env[0] and falling from env[-1]."""
    env = np.asarray(env, dtype=np.float32)
    k = np.arange(p, dtype=np.float64)
    left = (k * (np.float64(env[0]) / p)).astype(np.float32)
    right = (k * (np.float64(env[-1]) / p)).astype(np.float32)[::-1]
    return np.concatenate([left, env, right])


def tempogram_direct(env, win):
    """Autocorrelation tempogram [win, n]: frame t is the ramp-padded envelope [t, t + win) times the periodic Hann(win); all lags by
    np.correlate in float64; each frame divided by its largest |value| (left alone when that is below float64's tiny)."""
    env = np.asarray(env, dtype=np.float32)
    n = len(env)
    padded = ramp_padded(env, win // 2).astype(np.float64)
    w = hann_periodic(win)
    out = np.empty((win, n), dtype=np.float64)
    for t in range(n):
        y = padded[t: t + win] * w
        ac = np.correlate(y, y, mode="full")[win - 1:]
        nrm = np.max(np.abs(ac))
        out[:, t] = ac / (1.0 if nrm < F64_TINY else nrm)
    return out


def yin_periods(sr, fmin, fmax, frame_length):
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - frame_length // 2 - 1)
    return min_period, max_period


def cmnd_direct(x, sr, fmin, fmax, frame_length, hop):
    """YIN's cumulative-mean-normalised difference [frames, lags min_period .. max_period] over centred frames (W = frame_length / 2):
    acf[tau] = sum_{j=1..W} y_j y_{j+tau} directly in float64; windowed energies from a sequential float32 cumulative sum of the
    squared frame; |acf| and |energy| under 1e-6 snapped to zero; d = (e[0] + e[tau]) - 2 acf; d / (running mean of d[1..tau] + tiny)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    W = frame_length // 2
    min_period, max_period = yin_periods(sr, fmin, fmax, frame_length)
    nf = 1 + n // hop
    xp = np.concatenate([np.zeros(W, np.float32), x, np.zeros(W + frame_length, np.float32)])
    out = np.empty((nf, max_period - min_period + 1), dtype=np.float64)
    for f in range(nf):
        y32 = xp[f * hop: f * hop + frame_length]
        y = y32.astype(np.float64)
        acf = np.correlate(y[1: W + 1 + max_period], y[1: W + 1], mode="valid")           # lags 0 .. max_period
        acf[np.abs(acf) < 1e-6] = 0.0
        cs = np.cumsum(y32 * y32, dtype=np.float32)                     # np.cumsum adds in index order, one float32 rounding per step
        e = cs[W: W + max_period + 1] - cs[: max_period + 1]
        e[np.abs(e) < np.float32(1e-6)] = np.float32(0.0)
        d = (e[0] + e).astype(np.float64) - 2.0 * acf
        run64 = 0.0
        cm = np.zeros(max_period + 1, dtype=np.float64)
        for tau in range(1, max_period + 1):
            run64 += d[tau]
            cm[tau] = d[tau] / (run64 / tau + F64_TINY)
        out[f] = cm[min_period:]
    return out


def yin_pick(cmnd, min_period, threshold=0.1):
    """Period per frame from cmnd [frames, lags]: the first lag that is a trough (below its left neighbour, not above its right one;
    the first lag needs only to be below the second, the last one only below its left) and under the threshold, else the first
    global minimum; then the parabolic shift -b / a through the pick's neighbours, none at either end or where |b| >= |a|."""
    cmnd = np.asarray(cmnd, dtype=np.float64)
    out = np.empty(cmnd.shape[0], dtype=np.float64)
    L = cmnd.shape[1]
    for f, c in enumerate(cmnd):
        pick = -1
        for i in range(L):
            if i == 0:
                trough = L > 1 and c[0] < c[1]
            elif i == L - 1:
                trough = c[i] < c[i - 1]
            else:
                trough = c[i] < c[i - 1] and c[i] <= c[i + 1]
            if trough and c[i] < threshold:
                pick = i
                break
        if pick < 0:
            pick = int(np.argmin(c))
        shift = 0.0
        if 0 < pick < L - 1:
            a = c[pick + 1] + c[pick - 1] - 2.0 * c[pick]
            b = (c[pick + 1] - c[pick - 1]) / 2.0
            if not abs(b) >= abs(a):
                shift = -b / a
        out[f] = min_period + pick + shift
    return out
