/*
 * audiocut_finish.h — segment finishing on the device: fades at both ends of every exported segment and one gain per segment
 * (RMS normalisation), applied where the float32 track becomes sample bytes.  This is the C ABI of libaudiocut_finish.so (gfx950),
 * a small library of its own next to libaudiocut_hip.so: it takes no ac_ctx, keeps its own error text (acf_last_error) and
 * shares only the subtype codes AC_PACK_* and the word conversion of include/audiocut_hip_pack.h.
 *
 * The reference ships the settings (`quality_control.fade_in_duration`, `fade_out_duration`, `normalize_audio`, expert.yaml:105-107)
 * and the arithmetic (`AudioProcessor.apply_fade`, `AudioProcessor.normalize_audio`; fade first, then normalise,
 * quality_controller.py:750-757).
 *
 * The finished sample.  The track has `channels` planar rows; spans [s_k, e_k) are sorted, disjoint and inside [0, n_frames]
 * (the callers' precondition: the tables live on the device and are not checked here; the kernels clamp every bound to
 * [0, n_frames] and read and write nothing but their own frames whatever the tables hold).  With L = e - s, Fi = fade_in,
 * Fo = fade_out, frame f of span k has i = f - s_k, every channel alike:
 *   1. fade in, only if Fi > 0 and L > Fi: for i < Fi, v = float32(float64(x) * w_in[i]), w_in = linspace(0, 1, Fi) in float64:
 *      i * (1.0 / (Fi - 1)), the last weight exactly 1.0; [0.0] for Fi == 1;
 *   2. fade out, only if Fo > 0 and L > Fo: for i >= L - Fo, v = float32(float64(v) * w_out[i - (L - Fo)]), w_out =
 *      linspace(1, 0, Fo): j * (-1.0 / (Fo - 1)) + 1.0, product and sum rounded separately, the last weight exactly 0.0; [1.0]
 *      for Fo == 1.  Where both fades cover a frame, step 2 acts on step 1's float32 result;
 *   3. gain: y = v * g_k, one float32 product;
 *   4. word: the conversion of ac_pack_pcm for `subtype`.
 * A frame outside every span is written as ac_pack_pcm writes it.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok, negative =
 * AC_E_INVALID / AC_E_HIP with the text in acf_last_error(), thread-local).
 */
#ifndef AUDIOCUT_FINISH_H
#define AUDIOCUT_FINISH_H

#include "../audiocut_hip_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACF_ABI_VERSION 1

int acf_abi_version(void);
const char* acf_last_error(void);

/* 16 partials per span, the p-th contiguous sixteenth each, summed in a fixed order (the scheme of ac_segment_sumsq_peak):
 * sumsq [n_spans][16] float64 of the faded samples of steps 1-2, peak [n_spans][16] float32 max |v|; both channels together.
 * A sixteenth without frames gives 0.0 and 0.0f.  x as for acf_pack_spans.  One launch, a workgroup per (span, sixteenth). */
int acf_span_stats(const float* x, int64_t n_frames, int channels, int64_t row_stride, const int64_t* span_start,
                   const int64_t* span_end, int n_spans, int64_t fade_in, int64_t fade_out, double* sumsq, float* peak, void* stream);

/* steps 1-4 for every frame of the track; out [n_frames * channels * width], aligned as ac_pack_out_align(subtype) says.
 * x: a mono [n_frames] track (channels == 1; row_stride is not read) or a planar [2][row_stride] one (row_stride >= n_frames),
 * float32, 4-byte aligned; the wide loads under the conditions of ac_pack_pcm, else sample by sample.  gain [n_spans] float32.
 * 0 < n_frames < 2^40, n_spans > 0, fade_in >= 0, fade_out >= 0.  Nothing is written past the last sample byte.  One launch. */
int acf_pack_spans(const float* x, int64_t n_frames, int channels, int64_t row_stride, const int64_t* span_start,
                   const int64_t* span_end, const float* gain, int n_spans, int64_t fade_in, int64_t fade_out, int subtype,
                   unsigned char* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_FINISH_H */
