/*
 * audiocut_hip_beat.h — beat / bar analysis (`BeatAnalyzer`, the spectral-fusion chorus detection) extension of the C ABI of
 * libaudiocut_hip.so (gfx950).  The entry points below are exported by the same library as include/audiocut_hip.h, whose
 * declarations, conventions and ABI version (6) they leave unchanged; this header has a version of its own.
 *
 * The reference's `analyze_beats` (src/audio_cut/analysis/beat_analyzer.py:101-155) computes three framewise series of the
 * mix - RMS(2048, hop), spectral centroid and spectral bandwidth - and averages each of them per bar.  These kernels are
 * the two spectral series in one pass over the mix and the three per-bar means in one launch.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_BEAT_H
#define AUDIOCUT_HIP_BEAT_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_BEAT_ABI_VERSION 1

int ac_beat_abi_version(void);

/* librosa.feature.spectral_centroid and librosa.feature.spectral_bandwidth (p = 2, norm = True, the centroid of the same
 * spectrogram) of x[n] at n_fft 2048, centred, zero padded: n_frames == 1 + n / hop frames, both outputs float64 in Hz.
 * Per frame: float64 periodic Hann, float64 FFT, spectrum rounded to complex64, magnitudes S_k float32 (k = 0..1024);
 *   length    = sum_k S_k in float64, replaced by 1.0 when below FLT_MIN;     sn_k = (float)(S_k / length);
 *   centroid  = sum_k f_k * sn_k,                       f_k = k * sr / 2048   (the bits of ac_stft2048_spectral's centroid);
 *   bandwidth = sqrt(sum_k sn_k * (centroid - f_k)^2).
 * A digitally silent frame gives exactly 0.0 twice.  One workgroup per frame; nothing per-bin leaves the chip. */
int ac_stft2048_centroid_bandwidth(ac_ctx* ctx, const float* x, int64_t n, int hop, double sr, double* centroid_out,
                                   double* bandwidth_out, int64_t n_frames, void* stream);

/* Per-bar means of three framewise series that share their frame times: rms[n_rms] float32, centroid[n_spec] and
 * bandwidth[n_spec] float64, n_rms == n_spec.  Bar b owns the half-open frame range [bar_lo[b], bar_hi[b]) with
 * 0 <= bar_lo[b], bar_hi[b] <= n_rms; ranges may be empty, overlap or leave frames out.
 *   out[0 * n_bars + b] = mean of (double)rms over the range, out[1 * n_bars + b] of centroid, out[2 * n_bars + b] of
 *   bandwidth; 0.0 in all three rows for an empty range (bar_hi[b] <= bar_lo[b]).
 * One workgroup per bar, a fixed strided order and a fixed reduction tree: the same bits on every run.  One launch. */
int ac_bar_means3(ac_ctx* ctx, const float* rms, int64_t n_rms, const double* centroid, const double* bandwidth, int64_t n_spec,
                  const int64_t* bar_lo, const int64_t* bar_hi, int n_bars, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_BEAT_H */
