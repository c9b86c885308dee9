/*
 * audiocut_hip_export.h — the `vocal_separation` mode's stem writer, an extension of the C ABI of libaudiocut_hip.so (gfx950).
 * The entry points below are exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI
 * version (6) they leave unchanged; this header has a version of its own.
 *
 * The reference's `_process_vocal_separation_only` (src/vocal_smart_splitter/core/seamless_splitter.py:958-1036) separates a
 * track and writes the two stems.  Nothing but the WAV writer and three energy sums reads the stems in that mode, so this kernel
 * goes from the iSTFT output straight to the finished 24-bit PCM: the stem algebra and effective-region overlap-add of
 * ac_mdx_assemble_ola, the conversion of ac_pack_pcm24 and the sums of ac_sum_squares in one pass over the track, with no float
 * stem in memory.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_EXPORT_H
#define AUDIOCUT_HIP_EXPORT_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_EXPORT_ABI_VERSION 1

int ac_export_abi_version(void);

/* track: mono [n] (channels == 1) or planar stereo [2][n] (channels == 2) float32; wave [n_items][2][261120] float32 (the output
 * of ac_mdx_istft); the five chunk tables are those of ac_mdx_assemble_ola, eff_start and eff_end ascending.
 *
 * Stem values: exactly what ac_mdx_assemble_ola / ac_mdx_assemble_ola_stereo write - the same float32 operations in the same
 * order, per covering chunk in chunk order, divided by the count of covering chunks; 0 where no effective region covers a sample.
 *   channels == 1: the mono stems, (w0 + w1) * 0.5 and ((m - w0) + (m - w1)) * 0.5          -> 3 n bytes per stream
 *   channels == 2: the stereo stems, w_c and m_c - w_c per channel, frames interleaved L, R  -> 6 n bytes per stream
 * Each value becomes one little-endian 24-bit PCM word by ac_pack_pcm24's conversion (libsndfile's clipping one, NaN -> 0).
 * stem_out receives the network's stem, rest_out the mix minus it: which of the two is the vocal is the caller's to know.
 * Both must be 4-byte aligned and hold exactly that many bytes; nothing is written past them.
 *
 * partials [3][n_partials] float64: per-workgroup partial sums of squares of the MONO stem, the mono rest and the mono mix (for a
 * stereo track the mono stems of ac_mdx_assemble_ola_stereo and (L + R) * 0.5 in float32).  The caller adds each row in index
 * order: no atomics, every run gives the same bits.  n_partials in [1, 4096] is also the number of workgroups launched.
 * One launch. */
int ac_mdx_assemble_pcm24(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave, const int64_t* chunk_start,
                          const int64_t* chunk_len, const int64_t* eff_start, const int64_t* eff_end, const int32_t* item_base,
                          int n_chunks, unsigned char* stem_out, unsigned char* rest_out, double* partials, int n_partials,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_EXPORT_H */
