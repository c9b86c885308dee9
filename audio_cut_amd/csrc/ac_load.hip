// The loader's decode (include/audiocut_hip_load.h): the sample bytes of a RIFF/WAVE file, as they stand in the file, to the float32
// track the pipeline works on - the channel mean of `librosa.load(mono=True)` or planar channels.  The mirror image of the export
// end's k_pack_pcm / k_mdx_assemble_pcm.  A streaming kernel: 64 MB in, 42 MB out for four minutes of 24-bit stereo.
//
// Work split.  A frame is channels * width bytes, anything from 1 to 64, so neither "a frame per lane" (6-byte lanes: no dword
// alignment) nor "four frames per lane" (dword aligned, but a lane's span grows to 256 bytes and one load instruction of a wave then
// touches 64 different cache lines) reads the file the way memory wants it read.  So the two sides are decoupled through LDS:
//   * a workgroup owns AC_LOAD_FRAMES_PER_BLOCK consecutive frames and takes them in passes of 1024, 512 or 256 frames, the
//     largest whose bytes fit the 16 KB stage (1024 up to 16 bytes per frame: every 1- and 2-channel file but stereo float64);
//   * a pass's bytes are one contiguous, dword-aligned run of the file (a pass starts at a multiple of 256 frames and `bytes`
//     is 4-byte aligned): lane i copies dword i, i + 256, ... to LDS - ideal coalescing whatever the format - and the last
//     (bytes % 4) bytes of the file go bytewise, so nothing is read past the last byte;
//   * thread t then decodes frames t, t + 256, ... of the pass from LDS and stores out[frame] (mono) or out[c * stride + frame]
//     (planar): consecutive lanes write consecutive floats.
#include "ac_common.h"
#include "../../include/audiocut_hip_load.h"

#define AC_LOAD_STAGE_BYTES 16384      // >= 256 frames of the widest frame (8 channels x 8 bytes)

template <int FMT> struct ld_width { static constexpr int value = FMT == AC_LOAD_U8 ? 1 : FMT == AC_LOAD_S16 ? 2 : FMT == AC_LOAD_S24 ? 3 : FMT == AC_LOAD_F64 ? 8 : 4; };

// One sample at LDS address p (aligned to its width: the stage is 16-byte aligned and frame offsets are multiples of the width).
// Each is a single exact or once-rounded float32 operation, the one `decode_host` performs.
template <int FMT> __device__ inline float ld_sample(const unsigned char* p) {
    if constexpr (FMT == AC_LOAD_U8) {
        return (float)((int)p[0] - 128) / 128.0f;
    } else if constexpr (FMT == AC_LOAD_S16) {
        return (float)*reinterpret_cast<const short*>(p) / 32768.0f;
    } else if constexpr (FMT == AC_LOAD_S24) {
        const int v = (int)p[0] | ((int)p[1] << 8) | ((int)(signed char)p[2] * 65536);    // the top byte carries the sign
        return (float)v / 8388608.0f;
    } else if constexpr (FMT == AC_LOAD_S32) {
        return (float)*reinterpret_cast<const int*>(p) / 2147483648.0f;                  // v_cvt_f32_i32: nearest even
    } else if constexpr (FMT == AC_LOAD_F32) {
        return __uint_as_float(*reinterpret_cast<const unsigned*>(p));
    } else {
        return (float)*reinterpret_cast<const double*>(p);                               // v_cvt_f32_f64: nearest even, overflow -> inf
    }
}

template <int FMT>
__global__ __launch_bounds__(AC_LOAD_BLOCK) void k_decode_pcm(const unsigned char* __restrict__ bytes, int64_t n_frames, int channels,
                                                              int planar, float* __restrict__ out, int64_t out_stride,
                                                              unsigned long long* __restrict__ nonfinite) {
    constexpr int W = ld_width<FMT>::value;
    constexpr bool is_float = FMT == AC_LOAD_F32 || FMT == AC_LOAD_F64;
    __shared__ __attribute__((aligned(16))) unsigned s_raw[AC_LOAD_STAGE_BYTES / 4];
    unsigned char* s_bytes = reinterpret_cast<unsigned char*>(s_raw);
    const int tid = threadIdx.x;
    const int fb = channels * W;                                         // bytes per frame, <= 64
    const int pass = fb <= 16 ? 1024 : (fb <= 32 ? 512 : 256);           // frames per pass: pass * fb <= AC_LOAD_STAGE_BYTES
    const int64_t f_block = (int64_t)blockIdx.x * AC_LOAD_FRAMES_PER_BLOCK;
    const float fch = (float)channels;
    unsigned bad = 0u;
    for (int p0 = 0; p0 < AC_LOAD_FRAMES_PER_BLOCK; p0 += pass) {        // every condition below is uniform over the workgroup
        const int64_t f0 = f_block + p0;
        if (f0 >= n_frames) break;
        const int nf = n_frames - f0 < pass ? (int)(n_frames - f0) : pass;
        const int nb = nf * fb;                                          // <= AC_LOAD_STAGE_BYTES
        const unsigned char* __restrict__ src = bytes + f0 * fb;         // f0 % 256 == 0: dword aligned
        const unsigned* __restrict__ src32 = reinterpret_cast<const unsigned*>(src);
        const int nd = nb >> 2;
        for (int i = tid; i < nd; i += AC_LOAD_BLOCK) s_raw[i] = src32[i];
        if (tid < (nb & 3)) s_bytes[4 * nd + tid] = src[4 * nd + tid];   // only the last pass of the file can have such a tail
        __syncthreads();
        for (int j = tid; j < nf; j += AC_LOAD_BLOCK) {
            const unsigned char* fp = s_bytes + j * fb;
            const int64_t i = f0 + j;
            float acc = 0.f;
            for (int c = 0; c < channels; ++c) {
                const float v = ld_sample<FMT>(fp + c * W);
                if constexpr (is_float) bad += ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
                if (planar) out[(int64_t)c * out_stride + i] = v;
                else acc = c ? acc + v : v;
            }
            if (!planar) out[i] = channels > 1 ? acc / fch : acc;
        }
        __syncthreads();                                                 // the next pass overwrites the stage
    }
    if constexpr (is_float) {
        // every lane arrives here (no early return above): at most 4 * 8 per lane, 2048 per wave
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bad += (unsigned)__shfl_xor((int)bad, off, AC_WAVE);
        if ((tid & (AC_WAVE - 1)) == 0 && bad) atomicAdd(nonfinite, (unsigned long long)bad);
    }
}

extern "C" int ac_decode_pcm(ac_ctx* ctx, const unsigned char* bytes, int64_t n_frames, int channels, int sample_format, int layout,
                             float* out, int64_t out_stride, int64_t* nonfinite, void* stream) {
    AC_REQUIRE(ctx && bytes && out && nonfinite, "null pointer");
    AC_REQUIRE(n_frames > 0, "n_frames must be positive");
    AC_REQUIRE(channels >= 1 && channels <= AC_LOAD_MAX_CHANNELS, "channels must lie in 1..8");
    AC_REQUIRE(sample_format >= AC_LOAD_U8 && sample_format <= AC_LOAD_F64, "unknown sample format");
    AC_REQUIRE(layout == AC_LOAD_MONO || layout == AC_LOAD_PLANAR, "unknown layout");
    AC_REQUIRE((((uintptr_t)bytes) & 3) == 0, "bytes must be 4-byte aligned");
    AC_REQUIRE((((uintptr_t)out) & 3) == 0 && (((uintptr_t)nonfinite) & 7) == 0, "out must be 4-byte and nonfinite 8-byte aligned");
    AC_REQUIRE(layout == AC_LOAD_MONO || out_stride >= n_frames, "planar out_stride must not be below n_frames");
    const int64_t blocks = (n_frames + AC_LOAD_FRAMES_PER_BLOCK - 1) / AC_LOAD_FRAMES_PER_BLOCK;
    AC_REQUIRE(n_frames < (1LL << 41) && blocks < (1LL << 31), "track too long for one grid");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(nonfinite);
    AC_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
    const dim3 grid((unsigned)blocks), block(AC_LOAD_BLOCK);
    const int planar = layout == AC_LOAD_PLANAR;
    switch (sample_format) {
        case AC_LOAD_U8:  hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_U8>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
        case AC_LOAD_S16: hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_S16>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
        case AC_LOAD_S24: hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_S24>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
        case AC_LOAD_S32: hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_S32>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
        case AC_LOAD_F32: hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_F32>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
        default:          hipLaunchKernelGGL(k_decode_pcm<AC_LOAD_F64>, grid, block, 0, s, bytes, n_frames, channels, planar, out, out_stride, cnt); break;
    }
    AC_LAUNCH_CHECK();
    return AC_OK;
}
