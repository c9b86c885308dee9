/*
 * audiocut_hip_hybrid.h — the `hybrid_mdd` mode's quiet gate, an extension of the C ABI of libaudiocut_hip.so (gfx950).  The
 * entry points below are exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI version
 * (6) they leave unchanged; this header has a version of its own.
 *
 * The reference's `is_quiet_vocal_window` (src/vocal_smart_splitter/core/strategies/base.py:160-200) compares the RMS of a window
 * around one candidate beat with the 5th percentile of the RMS of the vocal stem's consecutive blocks, and recomputes those blocks
 * for every beat it is asked about.  This kernel reads the stem once: the mean square of every block and of the window around
 * every candidate, in one launch.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_HYBRID_H
#define AUDIOCUT_HIP_HYBRID_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_HYBRID_ABI_VERSION 1

int ac_hybrid_abi_version(void);

/* Mean squares of x[n] (float32) in float64, over consecutive blocks and over windows around given centres:
 *   block_ms[j]    = mean of (double)x[i]^2 over [j * half_win, min(n, (j + 1) * half_win)),  j < n_blocks == ceil(n / half_win);
 *                    the last block may be partial and is divided by its own length;
 *   point_count[k] = max(0, min(n, c + half_win) - max(0, c - half_win)),  c = centers[k];
 *   point_ms[k]    = mean over [max(0, c - half_win), min(n, c + half_win)), 0.0 when the count is 0.
 * Centres may be negative, at or beyond n, repeated, in any order.  half_win >= 1, n >= 0 (both below 2^40), n_centers >= 0;
 * n == 0 (then x may be NULL and n_blocks is 0) and n_centers == 0 are valid.
 * One wave per block or window: lane l adds elements lo + l, lo + l + 64, ... in float64, then a fixed shuffle tree; no atomics,
 * so every run gives the same bits, and a block and a window over the same samples give the same bits.  One launch. */
int ac_quiet_gate_meansq(ac_ctx* ctx, const float* x, int64_t n, int64_t half_win, const int64_t* centers, int n_centers,
                         double* block_ms, int64_t n_blocks, double* point_ms, int64_t* point_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_HYBRID_H */
