/*
 * audiocut_hip_asr.h — the `vpbd_asr` mode's ASR copy of the vocal stem, an extension of the C ABI of libaudiocut_hip.so (gfx950).
 * The entry points below are exported by the same library as include/audiocut_hip.h, whose declarations, conventions and ABI
 * version (6) they leave unchanged; this header has a version of its own.
 *
 * Before it asks a lyrics provider anything, the reference writes the separated vocal stem as a 16 kHz, 16-bit mono WAV
 * (src/vocal_smart_splitter/core/vocal_phrase_boundary_detector.py:388-411: librosa.resample, np.clip(-1, 1),
 * soundfile.write(subtype="PCM_16")).  The stem is resident in device memory, and nothing but the WAV writer reads the resampled
 * floats, so this kernel goes from the stem straight to the finished 16-bit PCM: the dot products of ac_resample_poly and the
 * conversion of the file writer in one pass, with no float stream in memory.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_ASR_H
#define AUDIOCUT_HIP_ASR_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_ASR_ABI_VERSION 1

int ac_asr_abi_version(void);

/* x [n] float32 at fs -> out [n_out] little-endian int16 at fs * up / down.  up, down, hp, hlen, n_pre_remove and n_out are
 * those of ac_resample_poly (hp = [up][hlen / up] polyphase rows), and the float every output is converted from is bit for bit
 * the one ac_resample_poly writes: the same one-wave-per-output dot product in float64 partial sums, the same reduction.
 *
 * Conversion: libsndfile's clipping float -> PCM_16 one (pcm.c f2les_clip_array, which python-soundfile selects on every file),
 * the 16-bit sibling of ac_pack_pcm24's: s = v * 2^31 in float32; s >= 2147483647.0f -> 0x7FFF; s <= -2^31 -> 0x8000; NaN -> 0;
 * else lrintf(s) >> 16.  It saturates at +-1, so the np.clip(-1, 1) the reference applies in front of the writer changes no
 * sample and is not a step of its own here.
 *
 * Stores: a wave's AC_RS_PER_WAVE = 8 consecutive outputs leave as ONE 16-byte store at byte offset 16 * (wave index).  `out`
 * must be 16-byte aligned and allocated for ceil(n_out / 8) * 8 samples; the samples of the last group past n_out are written
 * as zeros, nothing is written past the group.  One launch. */
int ac_resample_poly_pcm16(ac_ctx* ctx, const float* x, int64_t n, int up, int down, const float* hp, int64_t hlen,
                           int64_t n_pre_remove, int16_t* out, int64_t n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_ASR_H */
