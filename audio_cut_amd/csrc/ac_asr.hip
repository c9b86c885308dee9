// The `vpbd_asr` mode's ASR copy (include/audiocut_hip_asr.h): resident vocal stem -> 16 kHz 16-bit PCM in one pass.  The dot
// products are ac_polyphase_dot_wave (ac_common.h) with the arguments of k_resample_poly (ac_io.hip), so every float is the one
// that kernel writes; the conversion is pcm16() (ac_common.h), libsndfile's clipping one.  The float stream never reaches memory:
// this kernel replaces k_resample_poly, the download of its floats and the host's conversion on a path where only the WAV writer
// and the lyrics provider read the result.
#include "ac_common.h"
#include "../../include/audiocut_hip_asr.h"

extern "C" int ac_asr_abi_version(void) { return AC_ASR_ABI_VERSION; }

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
    AC_REQUIRE(n > 0 && up > 0 && down > 0 && hlen > 0 && n_pre_remove >= 0 && n_out > 0, "sizes must be positive");
    AC_REQUIRE(hlen % up == 0 && hlen / up < (1LL << 31), "hp is [up][hlen / up] polyphase rows");
    AC_REQUIRE((((uintptr_t)out) & 15) == 0, "out 16-byte aligned (and allocated for ceil(n_out / 8) * 8 samples)");
    const int64_t blocks = (n_out + 4 * AC_RS_PER_WAVE - 1) / (4 * AC_RS_PER_WAVE);
    AC_REQUIRE(blocks < (1LL << 31), "output too long");
    hipLaunchKernelGGL(k_resample_poly_pcm16, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, up, down, hp,
                       (int)(hlen / up), n_pre_remove, out, n_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
