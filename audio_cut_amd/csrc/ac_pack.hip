// The export end's sample formats (include/audiocut_hip_pack.h): the resident float32 track, or the iSTFT waves of the
// `vocal_separation` mode, -> finished WAV sample bytes of any of the six subtypes the loader reads (8-, 16-, 24- and 32-bit PCM,
// float32, float64).  Both kernels are streaming kernels: a thread owns a group of four words and a full group leaves as whole
// 32-bit or wider stores, consecutive threads writing consecutive groups (PCM_32 / FLOAT: 16 bytes per lane, 1 KiB per wave and
// instruction).  The integer words are the top bytes of pcm32() (ac_common.h), libsndfile's clipping conversion: python-soundfile
// switches libsndfile's clipping on (SFC_SET_CLIPPING), so soundfile.write(subtype="PCM_24") (`audio_export.py:109-111`) goes
// through pcm.c f2let_clip_array: s = x * 2^31 in float32; s >= 2^31 - 1 -> 0x7FFFFF, s <= -2^31 -> 0x800000, else the top three
// bytes of lrintf(s), i.e. lrintf(x * 2^31) >> 8 (a floor, not a rounding, of x * 2^23); the other integer subtypes likewise.
// The 24-bit entry points of include/audiocut_hip.h and include/audiocut_hip_export.h (ac_pack_pcm24, ac_mdx_assemble_pcm24) are
// the AC_PACK_PCM_24 instances of these kernels, kept at the end of this file.
#include "ac_common.h"
#include "../../include/audiocut_hip_export.h"
#include "../../include/audiocut_hip_pack.h"
#include "ac_pack_words.h"

#define MDX_ITEM 261120       // as in ac_mdx.hip
#define MDX_TRIM 3072
#define MDX_GEN 254976

extern "C" int ac_pack_width(int subtype) { return pk_width(subtype); }
extern "C" int ac_pack_out_align(int subtype) { return pk_align(subtype); }

// One thread per group.  VEC: the rows are aligned for the wide loads of a full group (the entry point decides); a partial group
// and an unaligned track are read sample by sample.  Every load is of frame f0 + j < n_frames of its row.
template <int CH, int ST, bool VEC>
__global__ __launch_bounds__(256) void k_pack_pcm(const float* __restrict__ x, int64_t n_frames, int64_t row_stride,
                                                  unsigned char* __restrict__ out) {
    constexpr int FR = 4 / CH;                          // frames per group
    const int64_t grp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f0 = grp * FR;
    if (f0 >= n_frames) return;
    const int frames = n_frames - f0 < FR ? (int)(n_frames - f0) : FR;
    float v[4];
    if (VEC && frames == FR) {
        if constexpr (CH == 1) {
            const float4 m = *reinterpret_cast<const float4*>(x + f0);
            v[0] = m.x; v[1] = m.y; v[2] = m.z; v[3] = m.w;
        } else {
            const float2 l = *reinterpret_cast<const float2*>(x + f0), r = *reinterpret_cast<const float2*>(x + row_stride + f0);
            v[0] = l.x; v[1] = r.x; v[2] = l.y; v[3] = r.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < FR; ++j) {
            if constexpr (CH == 1) {
                v[j] = j < frames ? x[f0 + j] : 0.f;
            } else {
                v[2 * j] = j < frames ? x[f0 + j] : 0.f;
                v[2 * j + 1] = j < frames ? x[row_stride + f0 + j] : 0.f;
            }
        }
    }
    ac_store_pcm_group<ST>(out, grp, v, frames * CH);
}

template <int CH, bool VEC>
static void pk_launch(int subtype, unsigned blocks, hipStream_t stream, const float* x, int64_t n_frames, int64_t row_stride,
                      unsigned char* out) {
#define PK_CASE(ST) case ST: hipLaunchKernelGGL((k_pack_pcm<CH, ST, VEC>), dim3(blocks), dim3(256), 0, stream, x, n_frames, row_stride, out); break
    switch (subtype) {
        PK_CASE(AC_PACK_PCM_U8); PK_CASE(AC_PACK_PCM_16); PK_CASE(AC_PACK_PCM_24); PK_CASE(AC_PACK_PCM_32); PK_CASE(AC_PACK_FLOAT);
        PK_CASE(AC_PACK_DOUBLE);
    }
#undef PK_CASE
}

extern "C" int ac_pack_pcm(ac_ctx* ctx, const float* x, int64_t n_frames, int channels, int64_t row_stride, int subtype,
                           unsigned char* out, void* stream) {
    AC_REQUIRE(ctx && x && out, "null pointer");
    AC_REQUIRE(n_frames > 0, "n_frames must be positive");
    AC_REQUIRE(n_frames < (1LL << 40), "track too long");
    AC_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    AC_REQUIRE(channels == 1 || row_stride >= n_frames, "row_stride must be at least n_frames");
    AC_REQUIRE(pk_width(subtype) != 0, "unknown subtype");
    AC_REQUIRE((((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
    AC_REQUIRE((((uintptr_t)out) & (uintptr_t)(pk_align(subtype) - 1)) == 0, "out must be aligned to ac_pack_out_align(subtype)");
    const int64_t groups = (n_frames * channels + 3) / 4;
    const unsigned blocks = (unsigned)((groups + 255) / 256);       // < 2^31: n_frames < 2^40
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 1) {
        if ((((uintptr_t)x) & 15) == 0) pk_launch<1, true>(subtype, blocks, s, x, n_frames, 0, out);
        else pk_launch<1, false>(subtype, blocks, s, x, n_frames, 0, out);
    } else {
        if ((((uintptr_t)x) & 7) == 0 && (row_stride & 1) == 0) pk_launch<2, true>(subtype, blocks, s, x, n_frames, row_stride, out);
        else pk_launch<2, false>(subtype, blocks, s, x, n_frames, row_stride, out);
    }
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// ---- the `vocal_separation` mode's stem writer for any subtype ---------------------------------------------------------------------
// iSTFT waves + resident track -> the two stems as finished sample bytes and the three energy sums of the confidence estimate, in
// one pass.  The stem values are those of k_mdx_assemble_ola (ac_mdx.hip) operation for operation and the sums are taken like
// k_sum_squares: this kernel replaces the launches of those and of the packing on a path where nobody reads the float stems.
// Templated on the channel count like k_mdx_assemble_ola, whose accumulation this repeats per frame: the covering chunks in chunk
// order, (w0 + w1) * 0.5 and ((m0 - w0) + (m1 - w1)) * 0.5 for the mono stems, w_c and m_c - w_c for the stereo ones, all divided
// by the chunk count.  The chunk tables are searched once per group, for its first frame: the chunks that cover a later frame of
// the group start at or after that index (eff_end ascends), and a chunk that does not hold a frame adds nothing to it, so every
// frame sees exactly the chunks, in the order, that the per-sample kernel gives it.
// Workgroup b walks groups b * 256 + t, + gridDim.x * 256, ...; its three float64 sums of squares (mono stem, mono rest, mono mix)
// go to partials[k * gridDim.x + b].  Only the two stores depend on the subtype ST.
template <int CH, int ST>
__global__ __launch_bounds__(256) void k_mdx_assemble_pcm(const float* __restrict__ track, int64_t n, const float* __restrict__ wave,
                                                          const int64_t* __restrict__ chunk_start,
                                                          const int64_t* __restrict__ chunk_len,
                                                          const int64_t* __restrict__ eff_start,
                                                          const int64_t* __restrict__ eff_end,
                                                          const int32_t* __restrict__ item_base, int n_chunks,
                                                          unsigned char* __restrict__ stem_out, unsigned char* __restrict__ rest_out,
                                                          double* __restrict__ partials) {
    constexpr int FR = 4 / CH;                          // frames per group
    __shared__ double s_red[4];
    const int64_t n_groups = (n + FR - 1) / FR;
    double e_stem = 0.0, e_rest = 0.0, e_mix = 0.0;
    for (int64_t grp = (int64_t)blockIdx.x * 256 + threadIdx.x; grp < n_groups; grp += (int64_t)gridDim.x * 256) {
        const int64_t g0 = grp * FR;
        const int frames = n - g0 < FR ? (int)(n - g0) : FR;
        int lo = 0, hi = n_chunks;                      // first chunk with eff_end > g0
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (eff_end[mid] > g0) hi = mid; else lo = mid + 1; }
        float m0[FR], m1[FR];
        if (CH == 1 && frames == FR) {
            const float4 m = *reinterpret_cast<const float4*>(track + g0);      // 16-byte aligned: g0 % 4 == 0
            m0[0] = m.x; m0[1] = m.y; m0[2] = m.z; m0[3] = m.w;
        } else {
#pragma unroll
            for (int j = 0; j < FR; ++j) m0[j] = j < frames ? track[g0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < FR; ++j) m1[j] = CH == 2 ? (j < frames ? track[n + g0 + j] : 0.f) : m0[j];
        float v_acc[FR], i_acc[FR], w_acc[FR], v0_acc[FR], v1_acc[FR], i0_acc[FR], i1_acc[FR];
#pragma unroll
        for (int j = 0; j < FR; ++j) v_acc[j] = i_acc[j] = w_acc[j] = v0_acc[j] = v1_acc[j] = i0_acc[j] = i1_acc[j] = 0.f;
        const int64_t g_last = g0 + frames - 1;
        for (int c = lo; c < n_chunks && eff_start[c] <= g_last; ++c) {
            const int64_t es = eff_start[c], ee = eff_end[c], cs = chunk_start[c], cl = chunk_len[c];
            const int base = item_base[c];
#pragma unroll
            for (int j = 0; j < FR; ++j) {
                const int64_t g = g0 + j;
                if (j >= frames || es > g || ee <= g) continue;
                const int64_t q = g - cs;
                if (q < 0 || q >= cl) continue;
                const int item = base + (int)(q / MDX_GEN);
                const int pos = MDX_TRIM + (int)(q % MDX_GEN);
                const float w0 = wave[((size_t)item * 2 + 0) * MDX_ITEM + pos];
                const float w1 = wave[((size_t)item * 2 + 1) * MDX_ITEM + pos];
                const float vocal = (w0 + w1) * 0.5f;
                const float inst = ((m0[j] - w0) + (m1[j] - w1)) * 0.5f;
                v_acc[j] += vocal;
                i_acc[j] += inst;
                w_acc[j] += 1.0f;
                if (CH == 2) {
                    v0_acc[j] += w0; v1_acc[j] += w1;
                    i0_acc[j] += m0[j] - w0; i1_acc[j] += m1[j] - w1;
                }
            }
        }
        float sv[4], rv[4];
#pragma unroll
        for (int j = 0; j < FR; ++j) {
            if (w_acc[j] == 0.f) w_acc[j] = 1.0f;
            const float v = v_acc[j] / w_acc[j], r = i_acc[j] / w_acc[j];
            if (CH == 1) {
                sv[j] = v; rv[j] = r;
            } else {
                sv[2 * j] = v0_acc[j] / w_acc[j]; sv[2 * j + 1] = v1_acc[j] / w_acc[j];
                rv[2 * j] = i0_acc[j] / w_acc[j]; rv[2 * j + 1] = i1_acc[j] / w_acc[j];
            }
            if (j < frames) {
                const float mm = CH == 2 ? (m0[j] + m1[j]) * 0.5f : m0[j];
                e_stem += (double)v * (double)v;
                e_rest += (double)r * (double)r;
                e_mix += (double)mm * (double)mm;
            }
        }
        ac_store_pcm_group<ST>(stem_out, grp, sv, frames * CH);
        ac_store_pcm_group<ST>(rest_out, grp, rv, frames * CH);
    }
    const double t_stem = block_sum_f64_256(e_stem, s_red);
    const double t_rest = block_sum_f64_256(e_rest, s_red);
    const double t_mix = block_sum_f64_256(e_mix, s_red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t_stem;
        partials[(size_t)gridDim.x + blockIdx.x] = t_rest;
        partials[2 * (size_t)gridDim.x + blockIdx.x] = t_mix;
    }
}

extern "C" int ac_mdx_assemble_pcm(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave,
                                   const int64_t* chunk_start, const int64_t* chunk_len, const int64_t* eff_start,
                                   const int64_t* eff_end, const int32_t* item_base, int n_chunks, int subtype,
                                   unsigned char* stem_out, unsigned char* rest_out, double* partials, int n_partials, void* stream) {
    AC_REQUIRE(ctx && track && wave && chunk_start && chunk_len && eff_start && eff_end && item_base && stem_out && rest_out && partials,
               "null pointer");
    AC_REQUIRE(n > 0 && n_chunks > 0, "sizes must be positive");
    AC_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    AC_REQUIRE(n < (1LL << 40), "track too long");
    AC_REQUIRE(pk_width(subtype) != 0, "unknown subtype");
    const uintptr_t mask = (uintptr_t)(pk_align(subtype) - 1);
    AC_REQUIRE((((uintptr_t)stem_out) & mask) == 0 && (((uintptr_t)rest_out) & mask) == 0,
               "out pointers must be aligned to ac_pack_out_align(subtype)");
    AC_REQUIRE(channels == 2 || (((uintptr_t)track) & 15) == 0, "a mono track must be 16-byte aligned");
    AC_REQUIRE(n_partials >= 1 && n_partials <= 4096, "n_partials must be in [1, 4096]");
#define PK_CASE(CH, ST)                                                                                                            \
    case ST:                                                                                                                       \
        hipLaunchKernelGGL((k_mdx_assemble_pcm<CH, ST>), dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, track, n, \
                           wave, chunk_start, chunk_len, eff_start, eff_end, item_base, n_chunks, stem_out, rest_out, partials);  \
        break
    if (channels == 1) {
        switch (subtype) {
            PK_CASE(1, AC_PACK_PCM_U8); PK_CASE(1, AC_PACK_PCM_16); PK_CASE(1, AC_PACK_PCM_24); PK_CASE(1, AC_PACK_PCM_32);
            PK_CASE(1, AC_PACK_FLOAT); PK_CASE(1, AC_PACK_DOUBLE);
        }
    } else {
        switch (subtype) {
            PK_CASE(2, AC_PACK_PCM_U8); PK_CASE(2, AC_PACK_PCM_16); PK_CASE(2, AC_PACK_PCM_24); PK_CASE(2, AC_PACK_PCM_32);
            PK_CASE(2, AC_PACK_FLOAT); PK_CASE(2, AC_PACK_DOUBLE);
        }
    }
#undef PK_CASE
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// ---- the 24-bit entry points: the AC_PACK_PCM_24 instances under their older names ------------------------------------------------
// A mono stream of n samples.  The alignment asked of x makes this always k_pack_pcm<1, AC_PACK_PCM_24, true>: a float4 load and
// three dwords per thread, the last partial group byte by byte.
extern "C" int ac_pack_pcm24(ac_ctx* ctx, const float* x, int64_t n, unsigned char* out, void* stream) {
    AC_REQUIRE(ctx && x && out, "null pointer");
    AC_REQUIRE(n > 0, "n must be positive");
    AC_REQUIRE((((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 3) == 0, "x 16-byte and out 4-byte aligned");
    return ac_pack_pcm(ctx, x, n, 1, n, AC_PACK_PCM_24, out, stream);     // refuses n >= 2^40 ("track too long"): 4 TB of samples, out of reach
}

extern "C" int ac_mdx_assemble_pcm24(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave,
                                     const int64_t* chunk_start, const int64_t* chunk_len, const int64_t* eff_start,
                                     const int64_t* eff_end, const int32_t* item_base, int n_chunks, unsigned char* stem_out,
                                     unsigned char* rest_out, double* partials, int n_partials, void* stream) {
    return ac_mdx_assemble_pcm(ctx, track, n, channels, wave, chunk_start, chunk_len, eff_start, eff_end, item_base, n_chunks,
                               AC_PACK_PCM_24, stem_out, rest_out, partials, n_partials, stream);
}
