// The word of a sample and the store of a group of four words for the six export subtypes (include/audiocut_hip_pack.h), shared by
// the kernels that write finished sample bytes: k_pack_pcm and k_mdx_assemble_pcm (ac_pack.hip) and k_resample_poly_pack
// (ac_rate.hip).  The conversions themselves (pcm16, pcm24, pcm32) are in ac_common.h.
#pragma once
#include "ac_common.h"
#include "../../include/audiocut_hip_pack.h"

__host__ __device__ constexpr int pk_width(int st) {
    return st == AC_PACK_PCM_U8 ? 1 : st == AC_PACK_PCM_16 ? 2 : st == AC_PACK_PCM_24 ? 3
         : (st == AC_PACK_PCM_32 || st == AC_PACK_FLOAT) ? 4 : st == AC_PACK_DOUBLE ? 8 : 0;
}
__host__ __device__ constexpr int pk_align(int st) {
    return (st == AC_PACK_PCM_U8 || st == AC_PACK_PCM_24) ? 4 : st == AC_PACK_PCM_16 ? 8
         : (st == AC_PACK_PCM_32 || st == AC_PACK_FLOAT || st == AC_PACK_DOUBLE) ? 16 : 0;
}

// the word of one sample for the subtypes of up to four bytes, in the low bytes of the result
template <int ST>
__device__ inline unsigned pk_word(float v) {
    if constexpr (ST == AC_PACK_PCM_U8) return (unsigned)((pcm32(v) >> 24) + 128) & 0xFF;
    else if constexpr (ST == AC_PACK_PCM_16) return (unsigned)pcm16(v) & 0xFFFF;
    else if constexpr (ST == AC_PACK_PCM_24) return (unsigned)pcm24(v) & 0xFFFFFF;
    else if constexpr (ST == AC_PACK_PCM_32) return (unsigned)pcm32(v);
    else return __float_as_uint(v);
}

// A thread owns one group of a stream: four words = four mono samples, or two stereo frames (L, R, L, R), 4 * width bytes at
// out + group * 4 * width, which is aligned to pk_align(ST) when `out` is.  A full group leaves as one dword (PCM_U8), one 8-byte
// store (PCM_16), three dwords (PCM_24: 12 bytes, 4-byte aligned), one 16-byte store (PCM_32, FLOAT) or two (DOUBLE); only the
// last group of a track can be partial (count < 4) and leaves byte by byte, so nothing is written past the last word.
template <int ST>
__device__ inline void ac_store_pcm_group(unsigned char* __restrict__ out, int64_t group, const float* v, int count) {
    constexpr int W = pk_width(ST);
    unsigned char* o = out + group * (4 * W);
    if constexpr (ST == AC_PACK_DOUBLE) {
        if (count == 4) {
            double2* w = reinterpret_cast<double2*>(o);
            w[0] = make_double2((double)v[0], (double)v[1]);
            w[1] = make_double2((double)v[2], (double)v[3]);
        } else {
            for (int j = 0; j < count; ++j) {
                const unsigned long long a = (unsigned long long)__double_as_longlong((double)v[j]);
#pragma unroll
                for (int b = 0; b < 8; ++b) o[j * 8 + b] = (unsigned char)(a >> (8 * b));
            }
        }
    } else {
        if (count == 4) {
            const unsigned a = pk_word<ST>(v[0]), b = pk_word<ST>(v[1]), c = pk_word<ST>(v[2]), d = pk_word<ST>(v[3]);
            if constexpr (W == 1) {
                *reinterpret_cast<unsigned*>(o) = a | (b << 8) | (c << 16) | (d << 24);
            } else if constexpr (W == 2) {
                *reinterpret_cast<uint2*>(o) = make_uint2(a | (b << 16), c | (d << 16));
            } else if constexpr (W == 3) {
                unsigned* w = reinterpret_cast<unsigned*>(o);
                w[0] = a | (b << 24);
                w[1] = (b >> 8) | (c << 16);
                w[2] = (c >> 16) | (d << 8);
            } else {
                *reinterpret_cast<uint4*>(o) = make_uint4(a, b, c, d);
            }
        } else {
            for (int j = 0; j < count; ++j) {
                const unsigned a = pk_word<ST>(v[j]);
#pragma unroll
                for (int b = 0; b < W; ++b) o[j * W + b] = (unsigned char)(a >> (8 * b));
            }
        }
    }
}
