/*
 * audiocut_hip_profile.h — the AutoProfile layer's one full-track computation, an extension of the C ABI of libaudiocut_hip.so
 * (gfx950).  The entry points below are exported by the same library as include/audiocut_hip.h, whose declarations, conventions
 * and ABI version (6) they leave unchanged; this header has a version of its own.
 *
 * AutoProfile estimates a track's style from four track-global features.  Three of them are in the feature cache already; the
 * fourth, the vocal coverage, is the share of the vocal stem's samples whose magnitude reaches 3 % of the stem's peak
 * (src/vocal_smart_splitter/core/seamless_splitter.py:873-893: peak = max |x|, threshold = max(0.03 * peak, 1e-5),
 * coverage = mean(|x| >= threshold)).  The stem is resident in device memory when the value is needed, so the peak and the
 * count are taken there: two streaming sweeps and 16 bytes to download.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_PROFILE_H
#define AUDIOCUT_HIP_PROFILE_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_PROFILE_ABI_VERSION 1

/* Launch shape of both sweeps: min(AC_PROFILE_MAX_BLOCKS, ceil(n / (4 * AC_PROFILE_BLOCK))) workgroups of AC_PROFILE_BLOCK threads;
 * a workgroup takes 4 * AC_PROFILE_BLOCK consecutive samples per step and strides over the signal.  The shape follows from n
 * alone, never from the device. */
#define AC_PROFILE_BLOCK 256
#define AC_PROFILE_MAX_BLOCKS 2048

int ac_profile_abi_version(void);

/* x [n] float32 (any 4-byte aligned address: a slice of a tensor is fine; read with dword loads), FINITE: no NaN, no infinity
 * (the stems are; with a NaN in the signal the results are unspecified).  0 <= n < 2^40.
 *
 *   *peak  (float32) = max_i |x[i]|                                   (+0.0 for an all-zero signal, -0.0 and denormals included)
 *   *thr   (float32) = (float) fmax((double) *peak * rel, abs_floor)  (rounded to float32 once, as numpy rounds the Python float
 *                                                                      it compares a float32 array with)
 *   *count (int64)   = #{ i : |x[i]| >= *thr }                        (compared in float32: a sample equal to the ROUNDED
 *                                                                      threshold counts even where that lies below the product)
 *
 * The three results are exact and independent of the order of evaluation: the maximum is an integer atomic maximum over the
 * magnitude bits (non-negative floats order as their bits do), the count an integer atomic sum of per-wave population counts.
 * Two calls on the same signal return the same bits.
 *
 * Everything is queued on `stream` with no host decision in between: the outputs are cleared, sweep 1 takes the peak, sweep 2
 * reads it from device memory, forms the threshold and counts.  With n == 0 the outputs are cleared (0.0f, 0.0f, 0) and
 * nothing else runs.  rel >= 0 and abs_floor >= 0. */
int ac_abs_peak_coverage(ac_ctx* ctx, const float* x, int64_t n, double rel, double abs_floor, float* peak, float* thr,
                         int64_t* count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_PROFILE_H */
