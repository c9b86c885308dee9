// The rational-rate polyphase FIR resamplers: three entry points around one device function,
// ac_polyphase_dot_wave (ac_common.h), one wave per output.
//  * ac_resample_poly: a resident track (the loader's 48 kHz -> 44.1 kHz, `audio_processor.py:45-49`).  The reference's
//    resampler is soxr_hq through librosa; libsoxr's coefficients are not available offline, so the host designs a low-pass to
//    soxr's published HQ specification (pass band to 0.9136 of the lower Nyquist, stop band from it, 126 dB: _native.py
//    `_resample_filter`) and hands it over in scipy.signal.resample_poly's framing (scaled by `up`, front-padded for alignment,
//    zero extension) as polyphase rows.
//  * ac_resample_poly_pcm16 (include/audiocut_hip_asr.h): the `vpbd_asr` mode's ASR copy, resident vocal stem -> 16 kHz 16-bit PCM
//    in one pass.  The dot products take the arguments of k_resample_poly, so every float is the one that kernel writes; the
//    conversion is pcm16() (ac_common.h), libsndfile's clipping one (pcm.c f2les_clip_array: python-soundfile switches
//    SFC_SET_CLIPPING on).  The float stream never reaches memory: this kernel replaces k_resample_poly, the download of its floats
//    and the host's conversion on a path where only the WAV writer and the lyrics provider read the result.
//  * ac_resample_poly_segments: every chunk's 44.1 kHz -> 16 kHz resampling in front of the Silero network (ac_vad.hip;
//    `vocal_pause_detector.py:189`) in one launch, written into a layout zero-padded per chunk to the 4096-sample bucket (`:192-196`).
#include "ac_common.h"
#include "../../include/audiocut_hip_asr.h"

// What ac_resample_poly and ac_resample_poly_pcm16 ask of their sizes, and the grid: four waves per workgroup, AC_RS_PER_WAVE
// outputs per wave.
static int rs_check_sizes(int64_t n, int up, int down, int64_t hlen, int64_t n_pre_remove, int64_t n_out, int64_t* n_blocks) {
    AC_REQUIRE(n > 0 && up > 0 && down > 0 && hlen > 0 && n_pre_remove >= 0 && n_out > 0, "sizes must be positive");
    AC_REQUIRE(hlen % up == 0 && hlen / up < (1LL << 31), "hp is [up][hlen / up] polyphase rows");
    const int64_t blocks = (n_out + 4 * AC_RS_PER_WAVE - 1) / (4 * AC_RS_PER_WAVE);
    AC_REQUIRE(blocks < (1LL << 31), "output too long");
    *n_blocks = blocks;
    return AC_OK;
}

__global__ __launch_bounds__(256) void k_resample_poly(const float* __restrict__ x, int64_t n, int up, int down,
                                                       const float* __restrict__ hp, int tpp, int64_t n_pre_remove,
                                                       float* __restrict__ out, int64_t n_out) {
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * AC_RS_PER_WAVE;      // a wave walks AC_RS_PER_WAVE consecutive outputs
    for (int64_t m = m0; m < m0 + AC_RS_PER_WAVE && m < n_out; ++m) {
        const float v = ac_polyphase_dot_wave(x, n, hp, up, tpp, (m + n_pre_remove) * (int64_t)down);
        if ((threadIdx.x & 63) == 0) out[m] = v;
    }
}

extern "C" int ac_resample_poly(ac_ctx* ctx, const float* x, int64_t n, int up, int down, const float* hp, int64_t hlen,
                                 int64_t n_pre_remove, float* out, int64_t n_out, void* stream) {
    AC_REQUIRE(ctx && x && hp && out, "null pointer");
    int64_t blocks;
    if (const int rc = rs_check_sizes(n, up, down, hlen, n_pre_remove, n_out, &blocks)) return rc;
    hipLaunchKernelGGL(k_resample_poly, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, up, down, hp,
                       (int)(hlen / up), n_pre_remove, out, n_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// A wave owns one group of AC_RS_PER_WAVE = 8 outputs = 16 bytes.  Every lane holds every sum (butterfly reduction), so the four
// words are assembled in registers without a shuffle and lane 0 stores them once.  Outputs past n_out stay 0 (wave-uniform test).
__global__ __launch_bounds__(256) void k_resample_poly_pcm16(const float* __restrict__ x, int64_t n, int up, int down,
                                                             const float* __restrict__ hp, int tpp, int64_t n_pre_remove,
                                                             int16_t* __restrict__ out, int64_t n_out) {
    static_assert(AC_RS_PER_WAVE == 8, "a group is eight int16 = one 16-byte store");
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * AC_RS_PER_WAVE;
    if (m0 >= n_out) return;                               // the last block's spare waves
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < AC_RS_PER_WAVE; ++j) {
        const int64_t m = m0 + j;
        if (m < n_out) {
            const float v = ac_polyphase_dot_wave(x, n, hp, up, tpp, (m + n_pre_remove) * (int64_t)down);
            w[j >> 1] |= ((unsigned)pcm16(v) & 0xFFFFu) << (16 * (j & 1));
        }
    }
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<uint4*>(out + m0) = make_uint4(w[0], w[1], w[2], w[3]);     // m0 % 8 == 0: 16-byte aligned
}

extern "C" int ac_resample_poly_pcm16(ac_ctx* ctx, const float* x, int64_t n, int up, int down, const float* hp, int64_t hlen,
                                       int64_t n_pre_remove, int16_t* out, int64_t n_out, void* stream) {
    AC_REQUIRE(ctx && x && hp && out, "null pointer");
    int64_t blocks;
    if (const int rc = rs_check_sizes(n, up, down, hlen, n_pre_remove, n_out, &blocks)) return rc;
    AC_REQUIRE((((uintptr_t)out) & 15) == 0, "out 16-byte aligned (and allocated for ceil(n_out / 8) * 8 samples)");
    hipLaunchKernelGGL(k_resample_poly_pcm16, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, up, down, hp,
                       (int)(hlen / up), n_pre_remove, out, n_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// Segmented polyphase resampling: ac_resample_poly for S independent segments in one launch.  Output m of segment s is
// sum_q hfull[(m + n_pre_remove) * down - q * up] x[in_off[s] + q] over the segment's own samples only (zero extension at its
// edges, as scipy.signal.resample_poly on the segment alone; taps as polyphase rows, ac_common.h); written at out[out_off[s] + m], m < out_len[s].
__global__ __launch_bounds__(256) void k_resample_poly_seg(const float* __restrict__ x, const int64_t* __restrict__ in_off,
                                                           const int64_t* __restrict__ in_len, const int64_t* __restrict__ out_off,
                                                           const int64_t* __restrict__ out_len, int n_seg, int up, int down,
                                                           const float* __restrict__ hp, int tpp, int64_t n_pre_remove,
                                                           float* __restrict__ out, int64_t n_work) {
    // a wave walks AC_RS_PER_WAVE consecutive indices of the concatenation of the segments' (bucket-padded) outputs
    const int64_t g0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * AC_RS_PER_WAVE;
    for (int64_t g = g0; g < g0 + AC_RS_PER_WAVE && g < n_work; ++g) {
        // out_off is increasing and segment s owns [out_off[s], out_off[s] + out_len[s]): binary search over the starts
        int lo = 0, hi = n_seg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (out_off[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const int64_t m = g - out_off[lo];
        if (m >= out_len[lo]) continue;                                   // bucket padding: stays zero
        const float v = ac_polyphase_dot_wave(x + in_off[lo], in_len[lo], hp, up, tpp, (m + n_pre_remove) * (int64_t)down);
        if ((threadIdx.x & 63) == 0) out[g] = v;
    }
}

extern "C" int ac_resample_poly_segments(ac_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                                         const int64_t* out_off, const int64_t* out_len, int n_seg, int up, int down,
                                         const float* h, int64_t hlen, int64_t n_pre_remove, float* out, int64_t n_out_total,
                                         void* stream) {
    AC_REQUIRE(ctx && x && in_off && in_len && out_off && out_len && h && out, "null pointer");
    AC_REQUIRE(n_seg > 0 && up > 0 && down > 0 && hlen > 0 && n_pre_remove >= 0 && n_out_total > 0, "sizes must be positive");
    AC_REQUIRE(hlen % up == 0 && hlen / up < (1LL << 31), "h is [up][hlen / up] polyphase rows");
    const int64_t blocks = (n_out_total + 4 * AC_RS_PER_WAVE - 1) / (4 * AC_RS_PER_WAVE);
    AC_REQUIRE(blocks < (1LL << 31), "output too long");
    hipLaunchKernelGGL(k_resample_poly_seg, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, in_off, in_len,
                       out_off, out_len, n_seg, up, down, h, (int)(hlen / up), n_pre_remove, out, n_out_total);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
