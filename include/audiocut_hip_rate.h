/*
 * audiocut_hip_rate.h — export at another sample rate (`output.sample_rate`), an extension of the C ABI of libaudiocut_hip.so
 * (gfx950).  The entry point below is exported by the same library as include/audiocut_hip.h, whose declarations, conventions and
 * ABI version (6) it leaves unchanged; this header has a version of its own.
 *
 * The pipeline runs at `audio.sample_rate` (44.1 kHz) and its stems are resident there.  A file that is to leave at another rate
 * (the rate of the input file: 48 or 96 kHz for a studio session) needs the stem resampled and converted to the sample format of
 * the WAV.  Nothing but the file writer reads the resampled floats, so this kernel goes from the resident stem straight to the
 * finished sample bytes: the dot products of ac_resample_poly and the conversion of ac_pack_pcm, declared in
 * include/audiocut_hip_pack.h, in one pass, with no float track at the output rate in memory.  It is the general form of
 * ac_resample_poly_pcm16, declared in include/audiocut_hip_asr.h: any of the six subtypes, mono or stereo, cropped to the frames
 * the caller keeps.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_RATE_H
#define AUDIOCUT_HIP_RATE_H

#include "audiocut_hip.h"
#include "audiocut_hip_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_RATE_ABI_VERSION 1

int ac_rate_abi_version(void);

/* x: a mono [n] track (channels == 1; row_stride is not read) or a planar [2][row_stride] track (channels == 2, row_stride >= n:
 * sample i of channel c is x[c * row_stride + i], so the rows may be views into wider rows), float32 at fs, 4-byte aligned.
 * up, down, hp, hlen and n_pre_remove are those of ac_resample_poly: hp = [up][hlen / up] polyphase rows.
 * subtype: one of the six AC_PACK_* codes.
 * out: the finished sample bytes at fs * up / down, n_out * channels * width of them (width: the subtype's ac_pack_width), stereo
 * frames interleaved L, R; aligned to the subtype's ac_pack_out_align, anything else is refused.  Nothing is written past the
 * last sample byte.
 * 1 <= n_out <= ceil(n * up / down): the caller's crop is a parameter, and nothing is computed for a frame that is not kept.
 *
 * The float each word is converted from is bit for bit the one ac_resample_poly writes for that channel and index - the same
 * one-wave-per-output dot product in float64 partial sums, the same reduction - and the conversion is that of ac_pack_pcm: the
 * bytes are those of ac_pack_pcm on the rows ac_resample_poly gives, cropped to n_out frames.
 *
 * A wave owns eight consecutive words of the stream (eight mono samples, or four stereo frames), which are two groups of
 * ac_pack_pcm; every lane holds every sum, and one lane stores a full group whole: one dword for PCM_U8 up to two 16-byte stores
 * for DOUBLE.  Only the last group of the track can be partial and leaves byte by byte.  One launch. */
int ac_resample_poly_pack(ac_ctx* ctx, const float* x, int64_t n, int channels, int64_t row_stride, int up, int down,
                          const float* hp, int64_t hlen, int64_t n_pre_remove, int subtype, unsigned char* out, int64_t n_out,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_RATE_H */
