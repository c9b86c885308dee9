/*
 * audiocut_hip_onset.h — bar-aligned smart segmentation (mode `librosa_onset`) extension of the C ABI of libaudiocut_hip.so
 * (gfx950).  The entry points below are exported by the same library as include/audiocut_hip.h, whose declarations,
 * conventions and ABI version (6) they leave unchanged; this header has a version of its own.
 *
 * The reference's `_process_librosa_onset_split` (src/vocal_smart_splitter/core/seamless_splitter.py:1038-1349) averages
 * the RMS(2048, hop) series of the mix per bar, flags its silent frames (:1100-1165) and labels every cut segment by the
 * energies of the two stems (:1252-1273).  These kernels are those reductions on the series and the stems resident in HBM.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_ONSET_H
#define AUDIOCUT_HIP_ONSET_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_ONSET_ABI_VERSION 1

int ac_onset_abi_version(void);

/* rms[n_frames] float32 (ac_frame_rms of the mix).  Bar b owns the half-open frame range [bar_lo[b], bar_hi[b]) with
 * 0 <= bar_lo[b], bar_hi[b] <= n_frames; ranges may be empty, overlap or leave frames out.
 *   bar_mean[b] = (sum of (double)rms[f] over the range) / count, 0.0 for an empty range (bar_hi[b] <= bar_lo[b]).  One
 *                 workgroup per bar, a fixed strided order and a fixed reduction tree: the same bits on every run.
 *   silent[f]   = 1 if 20 * log10((double)rms[f] + 1e-10) < threshold_db else 0, for every frame (uint8).
 * One launch. */
int ac_bar_energy_silence(ac_ctx* ctx, const float* rms, int64_t n_frames, const int64_t* bar_lo, const int64_t* bar_hi,
                          int n_bars, double threshold_db, double* bar_mean, uint8_t* silent, void* stream);

/* Sum of squares (float64) of vocal[a:b] and inst[a:b] for every segment [seg_start[s], seg_end[s]) inside [0, n], both
 * stems in one launch.  part_sumsq[n_seg][2][AC_PAIR_PARTS]: row 0 the vocal stem, row 1 the instrumental stem; entry p is
 * the fixed-order sum over the p-th contiguous sixteenth of the segment (ac_segment_sumsq_peak's scheme and bits), and the
 * caller adds the 16 entries in index order.  inst may be NULL: row 1 is then written as zeros.  An empty segment gives
 * zeros. */
#define AC_PAIR_PARTS 16
int ac_segment_pair_energy(ac_ctx* ctx, const float* vocal, const float* inst, int64_t n, const int64_t* seg_start,
                           const int64_t* seg_end, int n_seg, double* part_sumsq, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_ONSET_H */
