"""Plain float64 references of the MDX23 front and back end (audio_cut_amd/csrc/ac_mdx.hip) - TEST HELPER.  The transforms are
written from their definitions with numpy's float64 FFT: explicit reflect padding, explicit framing, an explicit overlap-add, where
the oracle calls torch.stft / torch.istft in float32.  Each comes with the scale a float32 evaluation's error is proportional to, so
that a quiet bin or a quiet frame is held to account like a loud one.  The table builders restate the plan -> table steps of
`MDX23HipBackend.separate_track`.  tests/test_mdx_kernels_gpu.py pins the transforms against torch in float64 on the CPU first."""
import numpy as np

from audio_cut_amd.separation.backends import items_per_chunk
from oracle import chunking as OC

N_FFT = OC.N_FFT          # 6144
HOP = OC.HOP              # 1024
T = OC.DIM_T              # 256
F = OC.DIM_F              # 3072
ITEM = OC.ITEM_LEN        # 261120
TRIM = OC.TRIM            # 3072
GEN = OC.GEN              # 254976
PADDED = HOP * (T - 1) + N_FFT


def hann64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def windowed_frames(items):
    """[B, 2, 261120] -> [B, 2, 256, 6144] float64: reflect padding of 3072 samples on each side, frames at hop 1024, periodic Hann."""
    x = np.asarray(items, dtype=np.float64)
    assert x.ndim == 3 and x.shape[1:] == (2, ITEM)
    xp = np.pad(x, ((0, 0), (0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    fr = np.lib.stride_tricks.sliding_window_view(xp, N_FFT, axis=-1)[:, :, ::HOP]
    assert fr.shape[2] == T
    return fr * hann64()


def stft64(items):
    """[B, 2, 261120] -> [B, 4 (L.re, L.im, R.re, R.im), 3072, 256] float64; bin 3072 is dropped."""
    z = np.fft.rfft(windowed_frames(items), axis=-1)[..., :F]                 # [B, 2, T, F]
    out = np.stack([z.real, z.imag], axis=2)                                  # [B, 2, 2, T, F]
    return np.ascontiguousarray(out.reshape(-1, 4, T, F).transpose(0, 1, 3, 2))


def stft_scale(items):
    """[B, 2, 256]: the L2 norm of each windowed frame.  A float32 FFT's error in ANY bin is proportional to this norm, not to the
    bin's own magnitude."""
    fr = windowed_frames(items)
    return np.sqrt(np.sum(fr * fr, axis=-1))


def _irfft_frames(spec):
    """[B, 4, 3072, 256] -> [B, 2, 256, 6144] float64: imaginary part of DC zeroed, bin 3072 zero, np.fft.irfft per frame."""
    s = np.asarray(spec, dtype=np.float64)
    assert s.ndim == 4 and s.shape[1:] == (4, F, T)
    s = s.reshape(-1, 2, 2, F, T)
    z = np.zeros((s.shape[0], 2, T, N_FFT // 2 + 1), dtype=np.complex128)
    z[..., :F] = (s[:, :, 0] + 1j * s[:, :, 1]).transpose(0, 1, 3, 2)
    z[..., 0] = z[..., 0].real
    return np.fft.irfft(z, n=N_FFT, axis=-1)


def ola_envelope():
    """sum_t hann^2 over the 256-frame lattice, in padded coordinates [0, 1024 * 255 + 6144)."""
    w2 = hann64() ** 2
    env = np.zeros(PADDED)
    for t in range(T):
        env[t * HOP: t * HOP + N_FFT] += w2
    return env


def _overlap_add(per_frame):
    """[B, 2, 256, 6144] (already windowed) -> [B, 2, 261120]: add over the padded length, divide by the envelope, cut the padding."""
    out = np.zeros(per_frame.shape[:2] + (PADDED,))
    for t in range(T):
        out[..., t * HOP: t * HOP + N_FFT] += per_frame[:, :, t]
    cut = slice(N_FFT // 2, N_FFT // 2 + ITEM)                                # the envelope is 0 at the two ends of the padded length
    return out[..., cut] / ola_envelope()[cut]


def istft64(spec):
    """[B, 4, 3072, 256] -> [B, 2, 261120] float64."""
    return _overlap_add(_irfft_frames(spec) * hann64())


def istft_scale(spec):
    """[B, 2, 261120]: sum_t rms(frame_t) * hann[p - 1024 t] / env[p] - the same overlap-add applied to each frame's level, so a
    sample between a loud and a quiet frame is judged by what actually contributes to it."""
    fr = _irfft_frames(spec)
    rms = np.sqrt(np.mean(fr * fr, axis=-1))                                  # [B, 2, T]
    return _overlap_add(rms[..., None] * hann64())


def ola_of_frame_levels(level):
    """[B, 2, 256] per-frame levels -> [B, 2, 261120]: sum_t level_t * hann[p - 1024 t] / env[p]."""
    return _overlap_add(np.asarray(level, dtype=np.float64)[..., None] * hann64())


def scaled_errors(got, ref, scale):
    """|got - ref| / scale element by element; 0 where the scale is 0 (what must hold there is exactness, which the caller asserts)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    sc = np.broadcast_to(scale, d.shape)
    return np.where(sc > 0.0, d / np.where(sc > 0.0, sc, 1.0), 0.0)


def scaled_error(got, ref, scale):
    """max |got - ref| / scale over the elements with scale > 0, and where it sits (an index tuple into `ref`)."""
    q = scaled_errors(got, ref, scale)
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), tuple(int(i) for i in at)


def per_frame(q):
    """Scaled errors (or scales) of a spectrum [B, 4, 3072, 256] -> their maximum per item and frame [B, 256]."""
    return np.max(q, axis=(1, 2))


def per_hop(q):
    """Scaled errors (or scales) of a wave [B, 2, 261120] -> their maximum per item and block of 1024 samples [B, 255]."""
    return np.max(q.reshape(q.shape[0], 2, -1, HOP), axis=(1, 3))


def spec_scale(items):
    """stft_scale shaped to divide a [B, 4, 3072, 256] spectrum: re and im of a channel share their frame's norm."""
    return np.repeat(stft_scale(items), 2, axis=1)[:, :, None, :]


# ---------------------------------------------------------------------------------------------------------------------
# plan -> tables (MDX23HipBackend.separate_track)
# ---------------------------------------------------------------------------------------------------------------------
def plan_ranges(n, sr=44100, **plan_args):
    """(chunk_start, chunk_end, eff_start, eff_end) of every non-empty chunk of an n-sample track."""
    ranges = OC.plan_sample_ranges(OC.chunk_plan(n / float(sr), **plan_args), sr, n)
    return [r for r in ranges if r[1] > r[0]]


def item_tables(ranges, align_hop=4096):
    """-> chunk_start int64, chunk_len int64, win_index int32: one entry per 261120-sample item, chunk after chunk."""
    cs_l, cl_l, wi_l = [], [], []
    for r in ranges:
        for k in range(items_per_chunk(r[1] - r[0], align_hop)):
            cs_l.append(r[0]); cl_l.append(r[1] - r[0]); wi_l.append(k)
    return np.asarray(cs_l, np.int64), np.asarray(cl_l, np.int64), np.asarray(wi_l, np.int32)


def chunk_tables(ranges, align_hop=4096):
    """-> chunk_start, chunk_len, eff_start, eff_end int64 and item_base int32 (the chunk's first item): one entry per chunk."""
    n_it = [items_per_chunk(r[1] - r[0], align_hop) for r in ranges]
    base = np.concatenate(([0], np.cumsum(n_it)[:-1])).astype(np.int32)
    col = lambda f: np.asarray([f(r) for r in ranges], np.int64)
    return col(lambda r: r[0]), col(lambda r: r[1] - r[0]), col(lambda r: r[2]), col(lambda r: r[3]), base


def coverage(n, ranges):
    """How many effective regions hold each of the n samples."""
    cnt = np.zeros(n, np.int64)
    for _, _, es, ee in ranges:
        if ee > es:
            cnt[es:ee] += 1
    return cnt


def restated_stereo_ola(x, wave, ranges, base, nbs):
    """Per channel: the effective-region overlap-add of w_c and m_c - w_c, summed in chunk order, divided by the count."""
    n = x.shape[1]
    v = np.zeros((2, n), np.float32); r = np.zeros((2, n), np.float32); cnt = np.zeros(n, np.float32)
    for c, (cs, ce, es, ee) in enumerate(ranges):
        if ee <= es:
            continue
        w = wave[base[c]:base[c] + nbs[c]][:, :, OC.TRIM:-OC.TRIM]
        w = w.transpose(1, 0, 2).reshape(2, -1)[:, es - cs: ee - cs]
        v[:, es:ee] += w
        r[:, es:ee] += x[:, es:ee] - w
        cnt[es:ee] += 1.0
    cnt[cnt == 0.0] = 1.0
    return v / cnt, r / cnt
