/*
 * audiocut_hip_load.h — the loader's decode, an extension of the C ABI of libaudiocut_hip.so (gfx950).  The entry points below
 * are exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI version (6) they leave
 * unchanged; this header has a version of its own.
 *
 * The export end writes stems as finished 24-bit PCM in one kernel (ac_mdx_assemble_pcm24, ac_pack_pcm24); this is its mirror
 * image at the input end.  The sample bytes of a RIFF/WAVE file go to the device as they stand in the file (3 bytes per sample of
 * a 24-bit file instead of 4 of the decoded float), and one kernel turns them into the float32 track the pipeline works on: the
 * channel mean of `librosa.load(mono=True)` (reference src/vocal_smart_splitter/utils/audio_processor.py:45-49) or the planar
 * channels of `audio.channels: 2`.  The header walk stays on the host (audio_cut_amd/utils/wav_reader.py), whose `decode_host` is
 * the numpy statement of the arithmetic below.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_LOAD_H
#define AUDIOCUT_HIP_LOAD_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_LOAD_ABI_VERSION 1

/* sample_format: the container of one sample, little-endian, left-justified (decoded by container width) */
#define AC_LOAD_U8 0  /* 1 byte,  unsigned:            (b - 128) / 128                                             */
#define AC_LOAD_S16 1 /* 2 bytes, two's complement:    v / 32768                                                   */
#define AC_LOAD_S24 2 /* 3 bytes, two's complement:    v / 8388608                                                 */
#define AC_LOAD_S32 3 /* 4 bytes, two's complement:    float32(v), rounded to nearest even, then / 2^31            */
#define AC_LOAD_F32 4 /* 4 bytes, IEEE binary32:       the bits as they are; nothing is clipped                    */
#define AC_LOAD_F64 5 /* 8 bytes, IEEE binary64:       rounded once to float32 (beyond its range: +-infinity)      */

/* layout */
#define AC_LOAD_MONO 0   /* out[i] = the channel mean of frame i                                                   */
#define AC_LOAD_PLANAR 1 /* out[c * out_stride + i] = channel c of frame i                                         */

#define AC_LOAD_MAX_CHANNELS 8

/* Launch shape: ceil(n_frames / AC_LOAD_FRAMES_PER_BLOCK) workgroups of AC_LOAD_BLOCK threads, one run of
 * AC_LOAD_FRAMES_PER_BLOCK consecutive frames each (no cap, no stride).  The shape follows from n_frames alone. */
#define AC_LOAD_BLOCK 256
#define AC_LOAD_FRAMES_PER_BLOCK 1024

int ac_load_abi_version(void);

/* bytes [n_frames * channels * width] interleaved sample bytes on the device, 4-byte aligned; nothing is read past the last byte.
 * 1 <= channels <= AC_LOAD_MAX_CHANNELS, 0 < n_frames < 2^41.
 *
 *   AC_LOAD_MONO:   out [n_frames] float32.  One channel: the sample.  More: the float32 sum of the samples in channel order
 *                   divided by float32(channels) - a division, not a product with a reciprocal.
 *   AC_LOAD_PLANAR: out [channels][out_stride] float32, out_stride >= n_frames; out[c * out_stride + i] for i < n_frames is
 *                   written and nothing else (the gaps between the rows keep their bytes).
 *
 * The values are exactly those of `decode_host` (wav_reader.py): every operation is one IEEE float32 operation with
 * denormals kept, in the same order.
 *
 *   *nonfinite (int64) = the number of input samples (every channel of every frame counts on its own) whose float32 value is NaN
 *                        or +-infinity; a binary64 sample beyond float32's range counts.  Always 0 for the integer formats.
 *
 * The call clears *nonfinite on `stream` and then launches one kernel; the count is an integer atomic sum of per-wave counts, so
 * it is exact and two calls on the same bytes return the same number.  A caller that goes on with the track checks it first:
 * with a non-zero count `out` holds NaNs or infinities (or means of them). */
int ac_decode_pcm(ac_ctx* ctx, const unsigned char* bytes, int64_t n_frames, int channels, int sample_format, int layout,
                  float* out, int64_t out_stride, int64_t* nonfinite, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_LOAD_H */
