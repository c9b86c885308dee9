// Bar-aligned smart segmentation (mode `librosa_onset`, include/audiocut_hip_onset.h): the two reductions of the reference's
// `_process_librosa_onset_split` (seamless_splitter.py:1100-1165, :1252-1273) on data resident in HBM.  Both are small and
// bandwidth-trivial (a 4-min track has ~20 k RMS frames; the stems are read once); what matters is a fixed summation order.
#include "ac_common.h"
#include "../../include/audiocut_hip_onset.h"

// (1) Blocks [0, n_bars): bar b's mean of rms[lo, hi) - thread t adds frames lo + t, lo + t + 256, ... in float64, then the wave
//     tree and the fixed sum of the four waves.  Blocks [n_bars, ...): one frame per thread, the silent flag in float64 from
//     the float32 RMS value (`20 * log10(rms + 1e-10) < threshold_db`, :1148-1149).
__global__ __launch_bounds__(256) void k_bar_energy_silence(const float* __restrict__ rms, int64_t n_frames,
                                                            const int64_t* __restrict__ bar_lo, const int64_t* __restrict__ bar_hi,
                                                            int n_bars, double threshold_db, double* __restrict__ bar_mean,
                                                            uint8_t* __restrict__ silent) {
    __shared__ double s_w[4];
    if ((int)blockIdx.x < n_bars) {
        const int b = blockIdx.x;
        int64_t lo = bar_lo[b], hi = bar_hi[b];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_frames ? n_frames : hi;
        double acc = 0.0;
        for (int64_t f = lo + threadIdx.x; f < hi; f += 256) acc += (double)rms[f];
        const double total = block_sum_f64_256(acc, s_w);
        if (threadIdx.x == 0) bar_mean[b] = hi > lo ? total / (double)(hi - lo) : 0.0;
        return;
    }
    const int64_t f = (int64_t)(blockIdx.x - n_bars) * 256 + threadIdx.x;
    if (f < n_frames) silent[f] = (20.0 * log10((double)rms[f] + 1e-10) < threshold_db) ? 1 : 0;
}

extern "C" int ac_bar_energy_silence(ac_ctx* ctx, const float* rms, int64_t n_frames, const int64_t* bar_lo, const int64_t* bar_hi,
                                      int n_bars, double threshold_db, double* bar_mean, uint8_t* silent, void* stream) {
    AC_REQUIRE(ctx && rms && bar_lo && bar_hi && bar_mean && silent, "null pointer");
    AC_REQUIRE(n_frames > 0 && n_bars > 0, "sizes must be positive");
    const int64_t flag_blocks = (n_frames + 255) / 256;
    AC_REQUIRE(flag_blocks + n_bars <= 0x7fffffff, "too many frames or bars");
    hipLaunchKernelGGL(k_bar_energy_silence, dim3((unsigned)(n_bars + flag_blocks)), dim3(256), 0, (hipStream_t)stream, rms, n_frames,
                       bar_lo, bar_hi, n_bars, threshold_db, bar_mean, silent);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// (2) k_segment_sumsq_peak's partials scheme (ac_guard.hip) on two stems at once: grid (segment, sixteenth), each workgroup
//     reads its sixteenth of both stems and writes one partial per stem; per stem the order of every addition is that
//     kernel's, so the partials are its bits.
__global__ __launch_bounds__(256) void k_segment_pair_energy(const float* __restrict__ vocal, const float* __restrict__ inst,
                                                             int64_t n, const int64_t* __restrict__ seg_start,
                                                             const int64_t* __restrict__ seg_end, double* __restrict__ part_sumsq) {
    __shared__ double s_v[4];
    __shared__ double s_i[4];
    const int s = blockIdx.x, part = blockIdx.y;
    int64_t a = seg_start[s], b = seg_end[s];
    a = a < 0 ? 0 : a;
    b = b > n ? n : b;
    b = b < a ? a : b;
    const int64_t chunk = (b - a + AC_PAIR_PARTS - 1) / AC_PAIR_PARTS;
    const int64_t lo = a + part * chunk, hi = (lo + chunk < b) ? lo + chunk : b;
    double av = 0.0, ai = 0.0;
    if (inst) {
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            const float v = vocal[i], w = inst[i];
            av += (double)v * (double)v;
            ai += (double)w * (double)w;
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { const float v = vocal[i]; av += (double)v * (double)v; }
    }
    av = wave_sum_f64(av);
    ai = wave_sum_f64(ai);
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = av; s_i[threadIdx.x >> 6] = ai; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* out = part_sumsq + (int64_t)s * 2 * AC_PAIR_PARTS;
        out[part] = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
        out[AC_PAIR_PARTS + part] = (s_i[0] + s_i[1]) + (s_i[2] + s_i[3]);
    }
}

extern "C" int ac_segment_pair_energy(ac_ctx* ctx, const float* vocal, const float* inst, int64_t n, const int64_t* seg_start,
                                       const int64_t* seg_end, int n_seg, double* part_sumsq, void* stream) {
    AC_REQUIRE(ctx && vocal && seg_start && seg_end && part_sumsq, "null pointer");
    AC_REQUIRE(n > 0 && n_seg > 0, "sizes must be positive");
    hipLaunchKernelGGL(k_segment_pair_energy, dim3((unsigned)n_seg, AC_PAIR_PARTS), dim3(256), 0, (hipStream_t)stream, vocal, inst, n,
                       seg_start, seg_end, part_sumsq);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
