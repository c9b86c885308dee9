// Beat / bar analysis (include/audiocut_hip_beat.h): the framewise spectral series and the per-bar reduction of the reference's
// `_compute_bar_features` (src/audio_cut/analysis/beat_analyzer.py:101-155) on the mix resident in HBM.
#include "ac_common.h"
#include "ac_fft2048.h"
#include "../../include/audiocut_hip_beat.h"

// (1) Spectral centroid and bandwidth per frame.  The frame, its FFT, the magnitudes and the centroid are k_stft2048_spectral's
//     (ac_fft2048.h: the same helpers in the same order, so the centroid has that kernel's bits); the magnitudes stay in LDS for a
//     third strided sweep, librosa.feature.spectral_bandwidth at p = 2: sqrt(sum_k sn_k * |f_k - centroid|^2), every term >= 0.
__global__ __launch_bounds__(256) void k_stft2048_centroid_bandwidth(const float* __restrict__ x, int64_t n, int hop, double sr,
                                                                     const double2* __restrict__ tw, const double* __restrict__ hann,
                                                                     double* __restrict__ centroid_out,
                                                                     double* __restrict__ bandwidth_out) {
    __shared__ double2 s_a[1024];
    __shared__ double2 s_b[1024];
    __shared__ float s_m[1025];
    __shared__ double s_red[16];
    const int64_t f = blockIdx.x;
    stft2048_load_frame(x, f * (int64_t)hop - 1024, 0, n, hann, s_a);
    const double2* Z = fft1024_f64(s_a, s_b, tw);
    stft2048_magnitudes(Z, tw, s_m);
    double length, lowsum, len_eff;
    const double centroid = stft2048_centroid(s_m, sr, s_red, &length, &lowsum, &len_eff);
    double v = 0.0;
    for (int k = threadIdx.x; k <= 1024; k += 256) {
        const float sn = stft2048_norm1(s_m[k], len_eff);
        const double d = fabs((double)k * sr / 2048.0 - centroid);
        v += (double)sn * (d * d);
    }
    const double var = block_sum_f64_256(v, s_red + 12);
    if (threadIdx.x == 0) {
        centroid_out[f] = centroid;
        bandwidth_out[f] = sqrt(var);
    }
}

extern "C" int ac_stft2048_centroid_bandwidth(ac_ctx* ctx, const float* x, int64_t n, int hop, double sr, double* centroid_out,
                                              double* bandwidth_out, int64_t n_frames, void* stream) {
    AC_REQUIRE(ctx && x && centroid_out && bandwidth_out, "null pointer");
    AC_REQUIRE(n > 0 && hop > 0 && n_frames == 1 + n / hop && n_frames < (1LL << 31), "n_frames != 1 + n/hop");
    hipLaunchKernelGGL(k_stft2048_centroid_bandwidth, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, x, n, hop, sr,
                       ctx->tw2048, ctx->hann2048, centroid_out, bandwidth_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// (2) One workgroup per bar: thread t adds frames lo + t, lo + t + 256, ... of each series in float64 (k_bar_energy_silence's
//     order), then the wave tree and the fixed sum of the four waves, once per series.  The range is clamped to the series: the
//     caller has checked it, the clamp keeps a wrong one from reading outside.
__global__ __launch_bounds__(256) void k_bar_means3(const float* __restrict__ rms, const double* __restrict__ centroid,
                                                    const double* __restrict__ bandwidth, int64_t n_frames,
                                                    const int64_t* __restrict__ bar_lo, const int64_t* __restrict__ bar_hi,
                                                    int n_bars, double* __restrict__ out) {
    __shared__ double s_w[12];
    const int b = blockIdx.x;
    int64_t lo = bar_lo[b], hi = bar_hi[b];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_frames ? n_frames : hi;
    double ar = 0.0, ac = 0.0, aw = 0.0;
    for (int64_t f = lo + threadIdx.x; f < hi; f += 256) {
        ar += (double)rms[f];
        ac += centroid[f];
        aw += bandwidth[f];
    }
    const double tr = block_sum_f64_256(ar, s_w);
    const double tc = block_sum_f64_256(ac, s_w + 4);
    const double tb = block_sum_f64_256(aw, s_w + 8);
    if (threadIdx.x == 0) {
        const bool any = hi > lo;
        const double cnt = (double)(hi - lo);
        out[b] = any ? tr / cnt : 0.0;
        out[(int64_t)n_bars + b] = any ? tc / cnt : 0.0;
        out[2 * (int64_t)n_bars + b] = any ? tb / cnt : 0.0;
    }
}

extern "C" int ac_bar_means3(ac_ctx* ctx, const float* rms, int64_t n_rms, const double* centroid, const double* bandwidth,
                             int64_t n_spec, const int64_t* bar_lo, const int64_t* bar_hi, int n_bars, double* out, void* stream) {
    AC_REQUIRE(ctx && rms && centroid && bandwidth && bar_lo && bar_hi && out, "null pointer");
    AC_REQUIRE(n_rms > 0 && n_bars > 0, "sizes must be positive");
    AC_REQUIRE(n_rms == n_spec, "the three series share their frame times");
    hipLaunchKernelGGL(k_bar_means3, dim3((unsigned)n_bars), dim3(256), 0, (hipStream_t)stream, rms, centroid, bandwidth, n_rms, bar_lo,
                       bar_hi, n_bars, out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
