// The `hybrid_mdd` mode's quiet gate (include/audiocut_hip_hybrid.h): the block and window mean squares behind the reference's
// `is_quiet_vocal_window` / `_vocal_floor_db` (src/vocal_smart_splitter/core/strategies/base.py:160-200) on the stem resident in HBM.
#include "ac_common.h"
#include "../../include/audiocut_hip_hybrid.h"

// One wave per job, four jobs per workgroup.  Jobs 0 .. n_blocks - 1 are the consecutive blocks, the rest the windows around the
// centres.  Lane l adds the squares of lo + l, lo + l + 64, ... (a coalesced 256-byte sweep per step) in float64, then the shuffle
// tree of wave_sum_f64: the order depends on (lo, hi) alone.  [lo, hi) is clamped to [0, n) whatever the centre is.
__global__ __launch_bounds__(256) void k_quiet_gate_meansq(const float* __restrict__ x, int64_t n, int64_t half_win,
                                                           const int64_t* __restrict__ centers, int64_t n_blocks, int64_t n_jobs,
                                                           double* __restrict__ block_ms, double* __restrict__ point_ms,
                                                           int64_t* __restrict__ point_count) {
    const int lane = threadIdx.x & (AC_WAVE - 1);
    const int64_t job = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= n_jobs) return;                          // wave-uniform
    int64_t lo = 0, hi = 0;
    if (job < n_blocks) {
        lo = job * half_win;
        hi = lo + half_win < n ? lo + half_win : n;
    } else {
        const int64_t c = centers[job - n_blocks];
        if (c > -half_win && c < n + half_win) {        // else the window misses the signal (and c +- half_win might overflow)
            lo = c - half_win > 0 ? c - half_win : 0;
            hi = c + half_win < n ? c + half_win : n;
        }
    }
    double acc = 0.0;
    for (int64_t i = lo + lane; i < hi; i += AC_WAVE) {
        const double v = (double)x[i];
        acc += v * v;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) {
        const int64_t cnt = hi > lo ? hi - lo : 0;
        const double ms = cnt > 0 ? acc / (double)cnt : 0.0;
        if (job < n_blocks) {
            block_ms[job] = ms;
        } else {
            point_ms[job - n_blocks] = ms;
            point_count[job - n_blocks] = cnt;
        }
    }
}

extern "C" int ac_quiet_gate_meansq(ac_ctx* ctx, const float* x, int64_t n, int64_t half_win, const int64_t* centers, int n_centers,
                                    double* block_ms, int64_t n_blocks, double* point_ms, int64_t* point_count, void* stream) {
    AC_REQUIRE(ctx, "null context");
    AC_REQUIRE(half_win >= 1 && half_win < (1LL << 40), "half_win must be at least 1");
    AC_REQUIRE(n >= 0 && n < (1LL << 40), "n must not be negative");
    AC_REQUIRE(n_centers >= 0, "n_centers must not be negative");
    AC_REQUIRE(n_blocks == (n + half_win - 1) / half_win, "n_blocks != ceil(n / half_win)");
    AC_REQUIRE(n == 0 || x, "null signal");
    AC_REQUIRE(n_blocks == 0 || block_ms, "null block output");
    AC_REQUIRE(n_centers == 0 || (centers && point_ms && point_count), "null centres or point outputs");
    const int64_t n_jobs = n_blocks + (int64_t)n_centers;
    if (n_jobs == 0) return AC_OK;
    const int64_t groups = (n_jobs + 3) / 4;
    AC_REQUIRE(groups < (1LL << 31), "too many blocks and centres for one launch");
    hipLaunchKernelGGL(k_quiet_gate_meansq, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, x, n, half_win, centers,
                       n_blocks, n_jobs, block_ms, point_ms, point_count);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
