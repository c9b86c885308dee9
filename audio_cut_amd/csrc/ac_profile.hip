// AutoProfile's vocal coverage (include/audiocut_hip_profile.h): the peak of |vocal stem| and the number of samples that reach 3 % of
// it (reference src/vocal_smart_splitter/core/seamless_splitter.py:873-893), on the stem resident in HBM.
#include "ac_common.h"
#include "../../include/audiocut_hip_profile.h"

// Magnitude bits of a float: for finite values they order exactly as |x| does (+-0 -> 0, denormals included), so the maximum and
// the comparison below are integer operations and do not depend on the float denormal mode.
__device__ inline unsigned pf_mag(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__global__ void k_profile_clear(float* __restrict__ peak, float* __restrict__ thr, unsigned long long* __restrict__ count) {
    if (threadIdx.x == 0) { *peak = 0.f; *thr = 0.f; *count = 0ULL; }
}

// Both sweeps walk the signal in tiles of AC_PROFILE_TILE = 4 * AC_PROFILE_BLOCK consecutive samples: workgroup g takes tiles g,
// g + gridDim.x, ...; thread t reads x[tile + t + 256 k], k < 4 (four independent coalesced dword loads in flight per lane).  The
// trip count is uniform over the workgroup.
#define AC_PROFILE_TILE (4 * AC_PROFILE_BLOCK)

// Sweep 1: max of the magnitude bits per lane, wave reduce, one atomicMax per wave.  Zeros are committed like any other value.
__global__ __launch_bounds__(AC_PROFILE_BLOCK) void k_profile_peak(const float* __restrict__ x, int64_t n, unsigned* __restrict__ peak_bits) {
    const int64_t stride = (int64_t)gridDim.x * AC_PROFILE_TILE;
    unsigned m = 0u;
    for (int64_t b = (int64_t)blockIdx.x * AC_PROFILE_TILE + threadIdx.x; b < n; b += stride) {
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = b + k * AC_PROFILE_BLOCK;
            v[k] = i < n ? pf_mag(x[i]) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) m = v[k] > m ? v[k] : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, AC_WAVE);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & (AC_WAVE - 1)) == 0) atomicMax(peak_bits, m);
}

// Sweep 2: the threshold from the finished peak, then the population count of (|x| >= thr) per wave and row, accumulated in a
// register; one 64-bit integer atomicAdd per wave.  Thread 0 of the grid stores the threshold.
__global__ __launch_bounds__(AC_PROFILE_BLOCK) void k_profile_count(const float* __restrict__ x, int64_t n, double rel, double abs_floor,
                                                                    const float* __restrict__ peak, float* __restrict__ thr,
                                                                    unsigned long long* __restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * AC_PROFILE_TILE;
    const float t = (float)fmax((double)*peak * rel, abs_floor);       // >= 0, finite
    const unsigned t_bits = __float_as_uint(t);
    if (blockIdx.x == 0 && threadIdx.x == 0) *thr = t;
    unsigned long long c = 0ULL;
    // the loop bound is taken on the wave's first lane, so every lane of a wave makes the same trips and the ballots are whole
    const int64_t first = (int64_t)blockIdx.x * AC_PROFILE_TILE + (threadIdx.x & ~(AC_WAVE - 1));
    const int lane = threadIdx.x & (AC_WAVE - 1);
    for (int64_t b = first; b < n; b += stride) {
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = b + lane + k * AC_PROFILE_BLOCK;
            hit[k] = i < n && pf_mag(x[i]) >= t_bits;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) c += (unsigned long long)__popcll(__ballot(hit[k]));
    }
    if (lane == 0 && c) atomicAdd(count, c);
}

extern "C" int ac_abs_peak_coverage(ac_ctx* ctx, const float* x, int64_t n, double rel, double abs_floor, float* peak, float* thr,
                                    int64_t* count, void* stream) {
    AC_REQUIRE(ctx, "null context");
    AC_REQUIRE(n >= 0 && n < (1LL << 40), "n must lie in [0, 2^40)");
    AC_REQUIRE(n == 0 || x, "null signal");
    AC_REQUIRE(peak && thr && count, "null output");
    AC_REQUIRE(rel >= 0.0, "rel must not be negative");
    AC_REQUIRE(abs_floor >= 0.0, "abs_floor must not be negative");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
    hipLaunchKernelGGL(k_profile_clear, dim3(1), dim3(AC_WAVE), 0, s, peak, thr, cnt);
    AC_LAUNCH_CHECK();
    if (n == 0) return AC_OK;
    int64_t blocks = (n + AC_PROFILE_TILE - 1) / AC_PROFILE_TILE;
    if (blocks > AC_PROFILE_MAX_BLOCKS) blocks = AC_PROFILE_MAX_BLOCKS;
    hipLaunchKernelGGL(k_profile_peak, dim3((unsigned)blocks), dim3(AC_PROFILE_BLOCK), 0, s, x, n, reinterpret_cast<unsigned*>(peak));
    AC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_profile_count, dim3((unsigned)blocks), dim3(AC_PROFILE_BLOCK), 0, s, x, n, rel, abs_floor, peak, thr, cnt);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
