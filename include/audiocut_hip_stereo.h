/*
 * audiocut_hip_stereo.h — true-stereo extension of the C ABI of libaudiocut_hip.so (gfx950).  The entry points below are
 * exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI version (6) they leave
 * unchanged; this header has a version of its own.
 *
 * The reference's MDX23OnnxBackend.infer_chunk accepts a (2, n) chunk and runs both channels through the network as they
 * are (src/audio_cut/separation/backends.py:268-281), then returns the channel means of `wave` and `mix - wave` (:389-406).
 * These kernels are that path for a resident stereo track; the U-Net and ac_mdx_istft already work on two channels.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 * A stereo track is PLANAR float32 [2][n]: row 0 = L, row 1 = R, the channel stride is n.  Chunk and item tables are the
 * ones the mono entry points take, and every chunk lies inside the track (chunk_start + chunk_len <= n).
 */
#ifndef AUDIOCUT_HIP_STEREO_H
#define AUDIOCUT_HIP_STEREO_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_STEREO_ABI_VERSION 1

int ac_stereo_abi_version(void);

/* ac_mdx_stft on both channels: channel c of track[2][n] -> spec_out channels 2c (re) and 2c+1 (im), i.e. L.re, L.im, R.re,
 * R.im of spec_out[n_items][4][256][3072] (T-major).  Per channel the arithmetic is ac_mdx_stft's, so L == R gives its
 * spectrum bit for bit.  spec_amax [n_items][256], zeroed by the caller, may be NULL: max |spec| per item and frame over all
 * four channels (order-independent atomicMax, deterministic). */
int ac_mdx_stft_stereo(ac_ctx* ctx, const float* track, int64_t n, const int64_t* chunk_start,
                       const int64_t* chunk_len, const int32_t* win_index, int n_items, float* spec_out,
                       float* spec_amax, void* stream);

/* ac_mdx_assemble_ola for a stereo mix track[2][n] and the network's wave[items][2][261120]: per covering chunk (chunk order)
 *   vocal = (w0 + w1) * 0.5,  inst = ((m0 - w0) + (m1 - w1)) * 0.5          (mdx_assemble's channel means)
 * summed over the effective regions and divided by their count -> vocal_out[n], inst_out[n]; in the same pass, per channel c,
 * w_c and m_c - w_c with the same sums and count -> vocal_st_out[2][n], inst_st_out[2][n] (each may be NULL: not written).
 * "vocal" is the network's stem: the caller swaps the pairs for an instrumental-type network. */
int ac_mdx_assemble_ola_stereo(ac_ctx* ctx, const float* track, int64_t n, const float* wave,
                               const int64_t* chunk_start, const int64_t* chunk_len, const int64_t* eff_start,
                               const int64_t* eff_end, const int32_t* item_base, int n_chunks,
                               float* vocal_out, float* inst_out, float* vocal_st_out, float* inst_st_out, void* stream);

/* ac_mdx_chunk_vocal for a stereo track: the per-chunk mono vocal (the chunked VAD input), chunk c at out[out_offset[c]],
 * (w0 + w1) * 0.5, or with mix_minus != 0 (instrumental-type network) ((m0 - w0) + (m1 - w1)) * 0.5 where m_c =
 * track[c][chunk_start + q].  track may be NULL when mix_minus == 0. */
int ac_mdx_chunk_vocal_stereo(ac_ctx* ctx, const float* track, int64_t n, const float* wave, const int64_t* chunk_start,
                              const int64_t* chunk_len, const int64_t* out_offset, const int32_t* item_base,
                              int n_chunks, int mix_minus, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_STEREO_H */
