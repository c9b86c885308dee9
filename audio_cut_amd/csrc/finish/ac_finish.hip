// libaudiocut_finish.so (include/finish/audiocut_finish.h): fades at both ends of every exported segment and one gain per segment,
// applied where the resident float32 track becomes sample bytes.  k_pack_spans is k_pack_pcm (../ac_pack.hip) with a span lookup:
// the same groups of four words, the same loads, the same stores (ac_store_pcm_group); k_span_stats gives the float64 sums of
// squares and the peaks of the FADED samples from which the host works out the gains.  Both call finish_fade(), so the sample that
// is measured is the sample that is written.  Float64 arithmetic runs in the fade zones alone; the interior of a span costs one
// float32 product per sample.  Built with -ffp-contract=off: the fade-out weight is a product and a sum rounded separately.
//
// Neither kernel trusts the span tables: every bound is clamped to [0, n_frames], a thread loads and stores only the frames of its
// own group (pack) or of its own clamped sixteenth (stats), and table reads are by an index in [0, n_spans).  Tables that break the
// header's preconditions (unsorted, overlapping) give bytes that mean nothing, never an access outside the buffers.
#include <stdarg.h>

#include "../ac_common.h"
#include "../ac_pack_words.h"
#include "../../../include/finish/audiocut_finish.h"

#define ACF_PARTS 16

static thread_local char g_acf_error[512] = "";

static int acf_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_acf_error, sizeof(g_acf_error), fmt, ap);
    va_end(ap);
    return code;
}

#define ACF_REQUIRE(cond, msg)                                                                       \
    do {                                                                                             \
        if (!(cond)) return acf_fail(AC_E_INVALID, "invalid argument: %s (%s)", msg, #cond);         \
    } while (0)

#define ACF_LAUNCH_CHECK()                                                                                                     \
    do {                                                                                                                       \
        hipError_t _e = hipGetLastError();                                                                                     \
        if (_e != hipSuccess) return acf_fail(AC_E_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

extern "C" int acf_abi_version(void) { return ACF_ABI_VERSION; }
extern "C" const char* acf_last_error(void) { return g_acf_error; }

__device__ inline int64_t acf_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

// Steps 1-2 of the header for the sample x at index i of a span of L frames.  The weights are numpy's linspace element for element:
// arange * step (+ start), the end point stored exactly.
__device__ inline float finish_fade(float x, int64_t i, int64_t L, int64_t Fi, int64_t Fo) {
    float v = x;
    if (Fi > 0 && L > Fi && i < Fi) {
        const double w = i == Fi - 1 ? (Fi == 1 ? 0.0 : 1.0) : (double)i * (1.0 / (double)(Fi - 1));
        v = (float)((double)v * w);
    }
    if (Fo > 0 && L > Fo && i >= L - Fo) {
        const int64_t j = i - (L - Fo);
        const double w = j == Fo - 1 ? (Fo == 1 ? 1.0 : 0.0) : (double)j * (-1.0 / (double)(Fo - 1)) + 1.0;
        v = (float)((double)v * w);
    }
    return v;
}

// One thread per group of four words, as k_pack_pcm.  A workgroup covers 1024 consecutive words.  Its threads first issue the loads
// of their samples, then read the span tables side by side - thread t takes spans t, t + 256, ... - and count the spans that end
// at or in front of the workgroup's first frame: for sorted spans that count is the index of the first span that can hold one of
// its frames (a ballot per wave, four partial counts through LDS, one barrier; no chain of dependent loads as a binary search
// has).  The first ACF_LDS_SPANS spans stay in LDS, clamped, with their gains, so the walk from that index to the span of a
// thread's own group reads LDS (no step at all in the common case of spans of seconds); spans behind them are read from memory.
// A group that lies wholly inside one span and outside its fade zones takes v * g; a group in a fade zone takes finish_fade() per
// frame; a group that straddles a span boundary (cuts fall on any sample) lets each frame find its own span.
#define ACF_LDS_SPANS 256
template <int CH, int ST, bool VEC>
__global__ __launch_bounds__(256) void k_pack_spans(const float* __restrict__ x, int64_t n_frames, int64_t row_stride,
                                                    const int64_t* __restrict__ span_start, const int64_t* __restrict__ span_end,
                                                    const float* __restrict__ gain, int n_spans, int64_t Fi, int64_t Fo,
                                                    unsigned char* __restrict__ out) {
    constexpr int FR = 4 / CH;                          // frames per group
    __shared__ int64_t s_end[ACF_LDS_SPANS], s_start[ACF_LDS_SPANS];
    __shared__ float s_gain[ACF_LDS_SPANS];
    __shared__ int s_part[4];
    const int64_t grp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f0 = grp * FR;
    const bool live = f0 < n_frames;                    // the last workgroup's spare threads load and store nothing
    const int frames = !live ? 0 : (n_frames - f0 < FR ? (int)(n_frames - f0) : FR);
    float v[4];
    if (VEC && frames == FR) {
        if constexpr (CH == 1) {
            const float4 m = *reinterpret_cast<const float4*>(x + f0);
            v[0] = m.x; v[1] = m.y; v[2] = m.z; v[3] = m.w;
        } else {
            const float2 l = *reinterpret_cast<const float2*>(x + f0), r = *reinterpret_cast<const float2*>(x + row_stride + f0);
            v[0] = l.x; v[1] = r.x; v[2] = l.y; v[3] = r.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < FR; ++j) {
            if constexpr (CH == 1) {
                v[j] = j < frames ? x[f0 + j] : 0.f;
            } else {
                v[2 * j] = j < frames ? x[f0 + j] : 0.f;
                v[2 * j + 1] = j < frames ? x[row_stride + f0 + j] : 0.f;
            }
        }
    }
    const int64_t w0 = (int64_t)blockIdx.x * 256 * FR;  // the workgroup's first frame
    int behind = 0;                                     // per wave: spans with end <= w0
    for (int base = 0; base < n_spans; base += 256) {   // the same trip count in every thread
        const int t = base + (int)threadIdx.x;
        bool ends_before = false;
        if (t < n_spans) {
            const int64_t e_t = acf_clamp(span_end[t], n_frames);
            ends_before = e_t <= w0;
            if (t < ACF_LDS_SPANS) { s_end[t] = e_t; s_start[t] = acf_clamp(span_start[t], n_frames); s_gain[t] = gain[t]; }
        }
        behind += __popcll(__ballot(ends_before));
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = behind;
    __syncthreads();
    if (!live) return;
    auto end_of = [&](int i) { return i < ACF_LDS_SPANS ? s_end[i] : acf_clamp(span_end[i], n_frames); };
    auto start_of = [&](int i) { return i < ACF_LDS_SPANS ? s_start[i] : acf_clamp(span_start[i], n_frames); };
    auto gain_of = [&](int i) { return i < ACF_LDS_SPANS ? s_gain[i] : gain[i]; };
    // the first span that ends behind f0, if any
    int k = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);     // <= n_spans whatever the tables hold
    int64_t s = 0, e = 0;
    for (; k < n_spans; ++k) {
        e = end_of(k);
        if (e > f0) { s = start_of(k); break; }
    }
    const int64_t f_last = f0 + frames - 1;
    if (k < n_spans && s <= f_last) {                   // else: outside every span, the words of k_pack_pcm
        if (s <= f0 && f_last < e) {                    // wholly inside span k
            const int64_t L = e - s, i0 = f0 - s;
            const float g = gain_of(k);
            const bool zone = (Fi > 0 && L > Fi && i0 < Fi) || (Fo > 0 && L > Fo && f_last - s >= L - Fo);
            if (!zone) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] * g;        // words past a partial group are not stored
            } else {
#pragma unroll
                for (int j = 0; j < FR; ++j) {
                    if (j < frames) {
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[j * CH + c] = finish_fade(v[j * CH + c], i0 + j, L, Fi, Fo) * g;
                    }
                }
            }
        } else {                                        // a boundary inside the group: frame by frame
#pragma unroll
            for (int j = 0; j < FR; ++j) {
                const int64_t f = f0 + j;
                if (j < frames) {
                    while (k < n_spans && e <= f) {
                        ++k;
                        if (k < n_spans) { e = end_of(k); s = start_of(k); }
                    }
                    if (k < n_spans && s <= f && f < e) {
                        const float g = gain_of(k);
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[j * CH + c] = finish_fade(v[j * CH + c], f - s, e - s, Fi, Fo) * g;
                    }
                }
            }
        }
    }
    ac_store_pcm_group<ST>(out, grp, v, frames * CH);
}

template <int CH, bool VEC>
static void ps_launch(int subtype, unsigned blocks, hipStream_t stream, const float* x, int64_t n_frames, int64_t row_stride,
                      const int64_t* span_start, const int64_t* span_end, const float* gain, int n_spans, int64_t fade_in,
                      int64_t fade_out, unsigned char* out) {
#define PS_CASE(ST)                                                                                                              \
    case ST:                                                                                                                     \
        hipLaunchKernelGGL((k_pack_spans<CH, ST, VEC>), dim3(blocks), dim3(256), 0, stream, x, n_frames, row_stride, span_start, \
                           span_end, gain, n_spans, fade_in, fade_out, out);                                                    \
        break
    switch (subtype) {
        PS_CASE(AC_PACK_PCM_U8); PS_CASE(AC_PACK_PCM_16); PS_CASE(AC_PACK_PCM_24); PS_CASE(AC_PACK_PCM_32); PS_CASE(AC_PACK_FLOAT);
        PS_CASE(AC_PACK_DOUBLE);
    }
#undef PS_CASE
}

extern "C" int acf_pack_spans(const float* x, int64_t n_frames, int channels, int64_t row_stride, const int64_t* span_start,
                              const int64_t* span_end, const float* gain, int n_spans, int64_t fade_in, int64_t fade_out, int subtype,
                              unsigned char* out, void* stream) {
    ACF_REQUIRE(x && span_start && span_end && gain && out, "null pointer");
    ACF_REQUIRE(n_frames > 0, "n_frames must be positive");
    ACF_REQUIRE(n_frames < (1LL << 40), "track too long");
    ACF_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    ACF_REQUIRE(channels == 1 || row_stride >= n_frames, "row_stride must be at least n_frames");
    ACF_REQUIRE(n_spans > 0, "n_spans must be positive");
    ACF_REQUIRE(fade_in >= 0 && fade_out >= 0, "fades must not be negative");
    ACF_REQUIRE(pk_width(subtype) != 0, "unknown subtype");
    ACF_REQUIRE((((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
    ACF_REQUIRE((((uintptr_t)out) & (uintptr_t)(pk_align(subtype) - 1)) == 0, "out must be aligned to ac_pack_out_align(subtype)");
    const int64_t groups = (n_frames * channels + 3) / 4;
    const unsigned blocks = (unsigned)((groups + 255) / 256);       // < 2^31: n_frames < 2^40
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 1) {
        if ((((uintptr_t)x) & 15) == 0) ps_launch<1, true>(subtype, blocks, s, x, n_frames, 0, span_start, span_end, gain, n_spans, fade_in, fade_out, out);
        else ps_launch<1, false>(subtype, blocks, s, x, n_frames, 0, span_start, span_end, gain, n_spans, fade_in, fade_out, out);
    } else {
        if ((((uintptr_t)x) & 7) == 0 && (row_stride & 1) == 0)
            ps_launch<2, true>(subtype, blocks, s, x, n_frames, row_stride, span_start, span_end, gain, n_spans, fade_in, fade_out, out);
        else ps_launch<2, false>(subtype, blocks, s, x, n_frames, row_stride, span_start, span_end, gain, n_spans, fade_in, fade_out, out);
    }
    ACF_LAUNCH_CHECK();
    return AC_OK;
}

// ---- the sums behind the gains ------------------------------------------------------------------------------------------------------
// grid (span, sixteenth): part p owns the p-th contiguous sixteenth of the span's frames, all channels of a frame; a thread adds its
// frames in ascending order, the workgroup in a fixed tree, the host the 16 parts in order: the same bits on every call.
__device__ inline float block_max_f32_256(float v, float* smem4) {
    v = wave_max_f32(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem4[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(smem4[0], smem4[1]), fmaxf(smem4[2], smem4[3]));
}

template <int CH>
__global__ __launch_bounds__(256) void k_span_stats(const float* __restrict__ x, int64_t n_frames, int64_t row_stride,
                                                    const int64_t* __restrict__ span_start, const int64_t* __restrict__ span_end,
                                                    int64_t Fi, int64_t Fo, double* __restrict__ part_sumsq,
                                                    float* __restrict__ part_peak) {
    __shared__ double s_s[4];
    __shared__ float s_p[4];
    const int span = blockIdx.x, part = blockIdx.y;
    const int64_t a = acf_clamp(span_start[span], n_frames), b = acf_clamp(span_end[span], n_frames);
    const int64_t L = b > a ? b - a : 0;
    const int64_t chunk = (L + ACF_PARTS - 1) / ACF_PARTS;
    const int64_t lo = a + part * chunk, hi = (lo + chunk < a + L) ? lo + chunk : a + L;    // lo <= a + 16 * chunk: no overflow
    double acc = 0.0;
    float pk = 0.f;
    for (int64_t f = lo + threadIdx.x; f < hi; f += 256) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float v = finish_fade(x[c * row_stride + f], f - a, L, Fi, Fo);
            acc += (double)v * (double)v;
            pk = fmaxf(pk, fabsf(v));
        }
    }
    const double total = block_sum_f64_256(acc, s_s);
    const float peak = block_max_f32_256(pk, s_p);
    if (threadIdx.x == 0) {
        part_sumsq[(int64_t)span * ACF_PARTS + part] = total;
        part_peak[(int64_t)span * ACF_PARTS + part] = peak;
    }
}

extern "C" int acf_span_stats(const float* x, int64_t n_frames, int channels, int64_t row_stride, const int64_t* span_start,
                              const int64_t* span_end, int n_spans, int64_t fade_in, int64_t fade_out, double* sumsq, float* peak,
                              void* stream) {
    ACF_REQUIRE(x && span_start && span_end && sumsq && peak, "null pointer");
    ACF_REQUIRE(n_frames > 0, "n_frames must be positive");
    ACF_REQUIRE(n_frames < (1LL << 40), "track too long");
    ACF_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    ACF_REQUIRE(channels == 1 || row_stride >= n_frames, "row_stride must be at least n_frames");
    ACF_REQUIRE(n_spans > 0, "n_spans must be positive");
    ACF_REQUIRE(fade_in >= 0 && fade_out >= 0, "fades must not be negative");
    ACF_REQUIRE((((uintptr_t)x) & 3) == 0, "x must be 4-byte aligned");
    const dim3 grid((unsigned)n_spans, ACF_PARTS);
    if (channels == 1)
        hipLaunchKernelGGL(k_span_stats<1>, grid, dim3(256), 0, (hipStream_t)stream, x, n_frames, (int64_t)0, span_start, span_end, fade_in,
                           fade_out, sumsq, peak);
    else
        hipLaunchKernelGGL(k_span_stats<2>, grid, dim3(256), 0, (hipStream_t)stream, x, n_frames, row_stride, span_start, span_end, fade_in,
                           fade_out, sumsq, peak);
    ACF_LAUNCH_CHECK();
    return AC_OK;
}
