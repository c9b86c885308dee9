// The `vocal_separation` mode's stem writer (include/audiocut_hip_export.h): iSTFT waves + resident track -> the two stems as
// finished 24-bit PCM and the three energy sums of the confidence estimate, in one pass.  The stem values are those of
// k_mdx_assemble_ola (ac_mdx.hip) operation for operation, the conversion is pcm24() of k_pack_pcm24 (ac_io.hip) and the sums are
// taken like k_sum_squares: this kernel replaces the launches of those three on a path where nobody reads the float stems.
#include "ac_common.h"
#include "../../include/audiocut_hip_export.h"

#define MDX_ITEM 261120       // as in ac_mdx.hip
#define MDX_TRIM 3072
#define MDX_GEN 254976

extern "C" int ac_export_abi_version(void) { return AC_EXPORT_ABI_VERSION; }

// A thread owns one 12-byte group of each stream: four PCM words = four mono samples, or two stereo frames (L, R, L, R).  Full
// groups leave as three 32-bit words like k_pack_pcm24's (a stream is 4-byte aligned and 12 * group is a multiple of 4); only the
// last group of a track can be partial (n % 4 samples, or the one frame of an odd stereo track) and leaves byte by byte.
__device__ inline void ac_store_pcm_group(unsigned char* __restrict__ out, int64_t group, const float* v, int count) {
    unsigned char* o = out + group * 12;
    if (count == 4) {
        const unsigned a = (unsigned)pcm24(v[0]) & 0xFFFFFF, b = (unsigned)pcm24(v[1]) & 0xFFFFFF;
        const unsigned c = (unsigned)pcm24(v[2]) & 0xFFFFFF, d = (unsigned)pcm24(v[3]) & 0xFFFFFF;
        unsigned* w = reinterpret_cast<unsigned*>(o);
        w[0] = a | (b << 24);
        w[1] = (b >> 8) | (c << 16);
        w[2] = (c >> 16) | (d << 8);
    } else {
        for (int j = 0; j < count; ++j) {
            const unsigned a = (unsigned)pcm24(v[j]) & 0xFFFFFF;
            o[j * 3] = (unsigned char)a; o[j * 3 + 1] = (unsigned char)(a >> 8); o[j * 3 + 2] = (unsigned char)(a >> 16);
        }
    }
}

// Templated on the channel count like k_mdx_assemble_ola, whose accumulation this repeats per frame: the covering chunks in chunk
// order, (w0 + w1) * 0.5 and ((m0 - w0) + (m1 - w1)) * 0.5 for the mono stems, w_c and m_c - w_c for the stereo ones, all divided
// by the chunk count.  The chunk tables are searched once per group, for its first frame: the chunks that cover a later frame of
// the group start at or after that index (eff_end ascends), and a chunk that does not hold a frame adds nothing to it, so every
// frame sees exactly the chunks, in the order, that the per-sample kernel gives it.
// Workgroup b walks groups b * 256 + t, + gridDim.x * 256, ...; its three float64 sums of squares (mono stem, mono rest, mono mix)
// go to partials[k * gridDim.x + b].
template <int CH>
__global__ __launch_bounds__(256) void k_mdx_assemble_pcm24(const float* __restrict__ track, int64_t n, const float* __restrict__ wave,
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
        ac_store_pcm_group(stem_out, grp, sv, frames * CH);
        ac_store_pcm_group(rest_out, grp, rv, frames * CH);
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

extern "C" int ac_mdx_assemble_pcm24(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave,
                                     const int64_t* chunk_start, const int64_t* chunk_len, const int64_t* eff_start,
                                     const int64_t* eff_end, const int32_t* item_base, int n_chunks, unsigned char* stem_out,
                                     unsigned char* rest_out, double* partials, int n_partials, void* stream) {
    AC_REQUIRE(ctx && track && wave && chunk_start && chunk_len && eff_start && eff_end && item_base && stem_out && rest_out && partials,
               "null pointer");
    AC_REQUIRE(n > 0 && n_chunks > 0, "sizes must be positive");
    AC_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    AC_REQUIRE(n < (1LL << 40), "track too long");
    AC_REQUIRE((((uintptr_t)stem_out) & 3) == 0 && (((uintptr_t)rest_out) & 3) == 0, "out pointers 4-byte aligned");
    AC_REQUIRE(channels == 2 || (((uintptr_t)track) & 15) == 0, "a mono track must be 16-byte aligned");
    AC_REQUIRE(n_partials >= 1 && n_partials <= 4096, "n_partials must be in [1, 4096]");
    if (channels == 1)
        hipLaunchKernelGGL(k_mdx_assemble_pcm24<1>, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, track, n, wave,
                           chunk_start, chunk_len, eff_start, eff_end, item_base, n_chunks, stem_out, rest_out, partials);
    else
        hipLaunchKernelGGL(k_mdx_assemble_pcm24<2>, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, track, n, wave,
                           chunk_start, chunk_len, eff_start, eff_end, item_base, n_chunks, stem_out, rest_out, partials);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
