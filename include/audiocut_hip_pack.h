/*
 * audiocut_hip_pack.h — the export end's sample formats, an extension of the C ABI of libaudiocut_hip.so (gfx950).  The entry
 * points below are exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI version (6)
 * they leave unchanged; this header has a version of its own.
 *
 * The reference exports with `soundfile.write(path, audio, sr, subtype=options["subtype"])`
 * (src/vocal_smart_splitter/utils/audio_export.py:109-111; the subtype is `output.wav.subtype`, config/unified.yaml:51).  The
 * loader reads every uncompressed WAV flavour (ac_decode_pcm, include/audiocut_hip_load.h); these two entry points write the same
 * six from the resident float32 track: ac_pack_pcm is ac_pack_pcm24 for any of them and does the stereo interleave itself,
 * ac_mdx_assemble_pcm is the ac_mdx_assemble_pcm24 of include/audiocut_hip_export.h for any of them.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_PACK_H
#define AUDIOCUT_HIP_PACK_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_PACK_ABI_VERSION 1

/* subtype: one little-endian word per sample.  v32(x) is the saturating conversion of ac_pack_pcm24: libsndfile's clipping
 * f2*_clip_array family, which python-soundfile switches on.  s = x * 2^31 in float32; s >= 2147483647.0f -> 0x7FFFFFFF,
 * s <= -2^31 -> -2^31, NaN -> 0, else s rounded half to even.  >> is the arithmetic shift. */
#define AC_PACK_PCM_U8 0 /* 1 byte,  unsigned: (v32 >> 24) + 128                                              */
#define AC_PACK_PCM_16 1 /* 2 bytes: v32 >> 16                                                                */
#define AC_PACK_PCM_24 2 /* 3 bytes: v32 >> 8 (ac_pack_pcm24's bytes)                                         */
#define AC_PACK_PCM_32 3 /* 4 bytes: v32                                                                      */
#define AC_PACK_FLOAT 4  /* 4 bytes: the float32 bits as they are; nothing clipped, NaN and infinities kept   */
#define AC_PACK_DOUBLE 5 /* 8 bytes: (double)x, exact                                                         */

int ac_pack_abi_version(void);

/* The byte width of a subtype's word (1, 2, 3, 4, 4, 8), or 0 for a value that is none of the six.  Host only. */
int ac_pack_width(int subtype);

/* The alignment in bytes that an output stream of `subtype` needs: that of the widest store a full group of four words leaves
 * as - 4 for PCM_U8 (one dword) and PCM_24 (three dwords), 8 for PCM_16 (one 8-byte store), 16 for PCM_32, FLOAT (one 16-byte
 * store) and DOUBLE (two).  0 for a value that is none of the six.  Host only. */
int ac_pack_out_align(int subtype);

/* x: a mono [n_frames] track (channels == 1; row_stride is not read) or a planar [2][row_stride] track (channels == 2,
 * row_stride >= n_frames: channel c of frame i is x[c * row_stride + i]), float32, 4-byte aligned.
 * out: the finished sample bytes, n_frames * channels * ac_pack_width(subtype) of them, stereo frames interleaved L, R; aligned to
 * ac_pack_out_align(subtype), anything else is refused.  Nothing is written past the last sample byte.  0 < n_frames < 2^40.
 *
 * A thread owns a group of four words (four mono samples, or two stereo frames) and stores a full group whole; only the last
 * group of a track can be partial and leaves byte by byte.  The loads are 16 bytes wide for a mono track that is 16-byte aligned
 * and 8 bytes per row for a stereo one whose two rows are 8-byte aligned (x 8-byte aligned and row_stride even); any other
 * track is read sample by sample - slower, never refused.  One launch; the interleave happens in the kernel. */
int ac_pack_pcm(ac_ctx* ctx, const float* x, int64_t n_frames, int channels, int64_t row_stride, int subtype, unsigned char* out,
                void* stream);

/* ac_mdx_assemble_pcm24 with the word of `subtype`: the same arguments, the same chunk search, the same float32 operations in the
 * same order for the stem values and the same three float64 partial rows (which do not depend on the subtype).  stem_out and
 * rest_out hold n * channels * ac_pack_width(subtype) bytes each, aligned to ac_pack_out_align(subtype); nothing is written past
 * them.  With AC_PACK_PCM_24 this is ac_mdx_assemble_pcm24, byte for byte.  One launch. */
int ac_mdx_assemble_pcm(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave, const int64_t* chunk_start,
                        const int64_t* chunk_len, const int64_t* eff_start, const int64_t* eff_end, const int32_t* item_base,
                        int n_chunks, int subtype, unsigned char* stem_out, unsigned char* rest_out, double* partials,
                        int n_partials, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_PACK_H */
