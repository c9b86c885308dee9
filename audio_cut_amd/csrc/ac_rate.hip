// Export at another sample rate (include/audiocut_hip_rate.h): the resident float32 stem at the pipeline rate -> finished WAV
// sample bytes of any of the six subtypes at fs * up / down, mono or interleaved stereo, in one launch.  The dot product is
// ac_polyphase_dot_wave (ac_common.h) with the arguments k_resample_poly (ac_polyphase.hip) gives it, so every float is the one
// that kernel writes for the channel and index; the word and the store are pk_word / ac_store_pcm_group (ac_pack_words.h), those of
// k_pack_pcm.  The float track at the output rate never reaches memory: this kernel replaces k_resample_poly per channel, the
// 4 bytes written and read again per sample, and k_pack_pcm on a path where only the file writer reads the result.  It is
// k_resample_poly_pcm16 for any subtype and channel count, with the caller's crop (n_out) as a parameter.
#include "ac_common.h"
#include "../../include/audiocut_hip_rate.h"
#include "ac_pack_words.h"

// A wave owns AC_RS_PER_WAVE = 8 consecutive words of the output stream, words w0 .. w0 + 7 with w0 % 8 == 0: eight mono samples,
// or four stereo frames L, R, L, R, .. (word w is channel w & 1 of frame w >> 1, and w & 1 == j & 1).  They are two groups of
// ac_store_pcm_group.  Every lane holds every sum (butterfly reduction), so lane 0 has both groups in registers and stores them:
// a full group whole, the track's last group byte by byte when it is partial.  `w < n_words` is the same in every lane, so the
// cross-lane reduction always runs with the whole wave; words past the crop are never computed.
template <int CH, int ST>
__global__ __launch_bounds__(256) void k_resample_poly_pack(const float* __restrict__ x, int64_t n, int64_t row_stride, int up, int down,
                                                            const float* __restrict__ hp, int tpp, int64_t n_pre_remove,
                                                            unsigned char* __restrict__ out, int64_t n_out) {
    static_assert(AC_RS_PER_WAVE == 8, "a wave's words are two groups of four");
    const int64_t n_words = n_out * CH;
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * AC_RS_PER_WAVE;
    if (w0 >= n_words) return;                             // the last block's spare waves
    float v[AC_RS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < AC_RS_PER_WAVE; ++j) {
        const int64_t w = w0 + j;
        v[j] = 0.f;
        if (w < n_words) {
            const int64_t m = CH == 2 ? (w >> 1) : w;
            const float* __restrict__ row = CH == 2 ? x + (j & 1) * row_stride : x;
            v[j] = ac_polyphase_dot_wave(row, n, hp, up, tpp, (m + n_pre_remove) * (int64_t)down);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t left = n_words - (w0 + 4 * g);
            if (left > 0) ac_store_pcm_group<ST>(out, w0 / 4 + g, v + 4 * g, left < 4 ? (int)left : 4);
        }
    }
}

template <int CH>
static void rp_launch(int subtype, unsigned blocks, hipStream_t stream, const float* x, int64_t n, int64_t row_stride, int up, int down,
                      const float* hp, int tpp, int64_t n_pre_remove, unsigned char* out, int64_t n_out) {
#define RP_CASE(ST) case ST: hipLaunchKernelGGL((k_resample_poly_pack<CH, ST>), dim3(blocks), dim3(256), 0, stream, x, n, row_stride, up, down, hp, tpp, n_pre_remove, out, n_out); break
    switch (subtype) {
        RP_CASE(AC_PACK_PCM_U8); RP_CASE(AC_PACK_PCM_16); RP_CASE(AC_PACK_PCM_24); RP_CASE(AC_PACK_PCM_32); RP_CASE(AC_PACK_FLOAT);
        RP_CASE(AC_PACK_DOUBLE);
    }
#undef RP_CASE
}

extern "C" int ac_resample_poly_pack(ac_ctx* ctx, const float* x, int64_t n, int channels, int64_t row_stride, int up, int down,
                                     const float* hp, int64_t hlen, int64_t n_pre_remove, int subtype, unsigned char* out, int64_t n_out,
                                     void* stream) {
    AC_REQUIRE(ctx && x && hp && out, "null pointer");
    AC_REQUIRE(n > 0 && up > 0 && down > 0 && hlen > 0 && n_pre_remove >= 0 && n_out > 0, "sizes must be positive");
    AC_REQUIRE(hlen % up == 0 && hlen / up < (1LL << 31), "hp is [up][hlen / up] polyphase rows");
    AC_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    AC_REQUIRE(channels == 1 || row_stride >= n, "row_stride must be at least n");
    AC_REQUIRE(n <= (1LL << 62) / up && n_pre_remove <= (1LL << 62) / down, "track too long");      // (m + n_pre_remove) * down fits
    AC_REQUIRE(n_out <= (n * up + down - 1) / down, "n_out must be at most ceil(n * up / down)");
    AC_REQUIRE(pk_width(subtype) != 0, "unknown subtype");
    AC_REQUIRE((((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
    AC_REQUIRE((((uintptr_t)out) & (uintptr_t)(pk_align(subtype) - 1)) == 0, "out must be aligned to ac_pack_out_align(subtype)");
    const int64_t blocks = (n_out * channels + 4 * AC_RS_PER_WAVE - 1) / (4 * AC_RS_PER_WAVE);
    AC_REQUIRE(blocks < (1LL << 31), "output too long");
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 1) rp_launch<1>(subtype, (unsigned)blocks, s, x, n, 0, up, down, hp, (int)(hlen / up), n_pre_remove, out, n_out);
    else rp_launch<2>(subtype, (unsigned)blocks, s, x, n, row_stride, up, down, hp, (int)(hlen / up), n_pre_remove, out, n_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
