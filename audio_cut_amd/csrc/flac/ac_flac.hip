// libaudiocut_flac.so (include/flac/audiocut_flac.h): FLAC frames from the finished PCM bytes on the device.  Two launches, one
// workgroup of 256 threads per frame: k_flac_plan chooses every frame's coding (the rules of utils/flac_export.py, integer
// arithmetic only) and counts its bytes exactly; after the host's exclusive scan of the lengths k_flac_write assembles each frame
// in an LDS bit buffer, adds both CRCs and copies it to its offset.
//
// Neither kernel trusts the frame table, and the write kernel trusts neither the records nor the offsets: every table entry is
// clamped to the track (acl_geometry), every record field to its range (order <= 4, p <= 6, k <= 30), every code is kept inside
// the LDS buffer (acl_put), and a frame is copied out only if its bytes are what its record promised and lie inside
// [0, total_bytes).  Plain C++ and vector stores only.
#include <stdarg.h>

#include "../ac_common.h"
#include "../../../include/flac/audiocut_flac.h"

#define ACL_MAX_BLOCK 4096
#define ACL_FINE 64                     // samples of the finest partition of a full block
#define ACL_BUF_WORDS 6400              // the frame's bit buffer: 25 600 bytes >= ACL_MAX_FRAME_BYTES
#define ACL_SUB 8                       // a subframe's fields inside a record
#define ACL_SUB_INTS 72
#define ACL_T_CONST 0
#define ACL_T_VERBATIM 1
#define ACL_T_FIXED 2

static thread_local char g_acl_error[512] = "";

static int acl_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_acl_error, sizeof(g_acl_error), fmt, ap);
    va_end(ap);
    return code;
}

#define ACL_REQUIRE(cond, msg)                                                                       \
    do {                                                                                             \
        if (!(cond)) return acl_fail(AC_E_INVALID, "invalid argument: %s (%s)", msg, #cond);         \
    } while (0)

#define ACL_LAUNCH_CHECK()                                                                                                     \
    do {                                                                                                                       \
        hipError_t _e = hipGetLastError();                                                                                     \
        if (_e != hipSuccess) return acl_fail(AC_E_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

extern "C" int acl_abi_version(void) { return ACL_ABI_VERSION; }
extern "C" const char* acl_last_error(void) { return g_acl_error; }

// ---- what both kernels share ------------------------------------------------------------------------------------------------
struct acl_geo {
    int64_t first;      // first frame of the track, in [0, n_frames]
    int bs;             // samples of this block, 0 = nothing to do
    int frame_no;       // < 2^21
    int pmax;           // the largest partition order: log2(block_size / 64) for a full block, else 0
};

__device__ inline acl_geo acl_geometry(const int64_t* __restrict__ table, int row, int64_t n_frames, int block_size) {
    acl_geo g;
    int64_t first = table[4 * (int64_t)row + 2], want = table[4 * (int64_t)row + 3];
    first = first < 0 ? 0 : (first > n_frames ? n_frames : first);
    const int64_t room = n_frames - first;
    int64_t bs = want < room ? want : room;
    bs = bs < block_size ? bs : block_size;
    g.first = first;
    g.bs = bs > 0 ? (int)bs : 0;
    g.frame_no = (int)(table[4 * (int64_t)row + 1] & 0x1FFFFF);
    g.pmax = 0;
    if (g.bs == block_size)
        for (int v = block_size / ACL_FINE; v > 1; v >>= 1) ++g.pmax;
    return g;
}

// the block's words as int32, channel by channel: bytes only, the track's byte offset has any residue
__device__ inline void acl_load_words(const unsigned char* __restrict__ pcm, const acl_geo& g, int channels, int width, int* sL, int* sR) {
    for (int i = threadIdx.x; i < g.bs; i += 256) {
        const unsigned char* p = pcm + (g.first + i) * (int64_t)(channels * width);
        for (int c = 0; c < channels; ++c, p += width) {
            int v;
            if (width == 2) v = (int)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
            else v = ((int)(((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16)) << 8)) >> 8;
            (c == 0 ? sL : sR)[i] = v;
        }
    }
}

// candidate signal c of the block: 0 L (or the mono channel), 1 R, 2 mid, 3 side
__device__ inline int acl_signal(const int* sL, const int* sR, int c, int i) {
    return c == 0 ? sL[i] : c == 1 ? sR[i] : c == 2 ? ((sL[i] + sR[i]) >> 1) : (sL[i] - sR[i]);
}

__device__ inline unsigned acl_fold(int r) { return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-(r + 1)) + 1u; }

// the smallest k with (n << k) >= S; S / n < 2^30, so k <= 30
__device__ inline int acl_rice_k(int64_t n, int64_t S) {
    int k = 0;
    while (k < 30 && (n << k) < S) ++k;
    return k;
}

__device__ inline int acl_header_bytes(int frame_no, int bs, int block_size) {
    const int num = frame_no < 128 ? 1 : frame_no < 2048 ? 2 : frame_no < 65536 ? 3 : 4;
    const int tail = bs == block_size ? 0 : (bs - 1 < 256 ? 1 : 2);
    return 4 + num + tail + 1;
}

__device__ inline int acl_block_sum_i32(int v, int* smem4) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (smem4[0] + smem4[1]) + (smem4[2] + smem4[3]);
}

// ---- plan ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_flac_plan(const unsigned char* __restrict__ pcm, int64_t n_frames, int channels, int width,
                                                   const int64_t* __restrict__ table, int block_size, int* __restrict__ records,
                                                   int* __restrict__ lengths) {
    __shared__ int sL[ACL_MAX_BLOCK], sR[ACL_MAX_BLOCK];
    __shared__ unsigned long long s_sum[5][ACL_FINE];       // per order, the sums of u over each run of 64 samples
    __shared__ long long s_est[35];
    __shared__ int s_k[ACL_FINE];
    __shared__ int s_pick[2];
    __shared__ int s_red[4];
    __shared__ int s_rec[4][ACL_SUB_INTS];
    __shared__ int s_bits[4];
    __shared__ int s_choice[4];
    const int row = blockIdx.x, t = threadIdx.x;
    int* rec = records + (int64_t)row * ACL_RECORD_INTS;
    const acl_geo g = acl_geometry(table, row, n_frames, block_size);
    if (g.bs == 0) {                                        // the same in every thread
        if (t < ACL_RECORD_INTS) rec[t] = 0;
        if (t == 0) lengths[row] = 0;
        return;
    }
    acl_load_words(pcm, g, channels, width, sL, sR);
    for (int j = t; j < 4 * ACL_SUB_INTS; j += 256) (&s_rec[0][0])[j] = 0;
    __syncthreads();
    const int bs = g.bs, bits = 8 * width;
    const int ncand = channels == 2 ? 4 : 1;
    const int maxo = bs - 1 < 4 ? bs - 1 : 4;
    const int nfine = (bs + ACL_FINE - 1) / ACL_FINE;       // 1 << pmax for a full block
    for (int c = 0; c < ncand; ++c) {
        const int bps = bits + (c == 3 ? 1 : 0);
        // constant?
        const int v0 = acl_signal(sL, sR, c, 0);
        int differs = 0;
        for (int i = t; i < bs; i += 256) differs |= acl_signal(sL, sR, c, i) != v0;
        if (!__syncthreads_or(differs)) {
            if (t == 0) { s_rec[c][0] = ACL_T_CONST; s_bits[c] = 8 + bps; }
            continue;                                       // uniform: the result of a barrier reduction
        }
        // the sums of u per run of 64 samples for the five orders: sample t + 256 j lies in run (t >> 6) + 4 j, which this wave owns
        for (int base = 0; base < nfine * ACL_FINE; base += 256) {
            const int i = base + t;
            unsigned u[5] = {0u, 0u, 0u, 0u, 0u};
            if (i < bs) {
                const int a0 = acl_signal(sL, sR, c, i);
                const int a1 = i >= 1 ? acl_signal(sL, sR, c, i - 1) : 0, a2 = i >= 2 ? acl_signal(sL, sR, c, i - 2) : 0;
                const int a3 = i >= 3 ? acl_signal(sL, sR, c, i - 3) : 0, a4 = i >= 4 ? acl_signal(sL, sR, c, i - 4) : 0;
                u[0] = acl_fold(a0);
                if (i >= 1 && maxo >= 1) u[1] = acl_fold(a0 - a1);
                if (i >= 2 && maxo >= 2) u[2] = acl_fold(a0 - 2 * a1 + a2);
                if (i >= 3 && maxo >= 3) u[3] = acl_fold(a0 - 3 * a1 + 3 * a2 - a3);
                if (i >= 4 && maxo >= 4) u[4] = acl_fold(a0 - 4 * a1 + 6 * a2 - 4 * a3 + a4);
            }
#pragma unroll
            for (int o = 0; o < 5; ++o) {
                unsigned lo = u[o] & 0xFFFFu, hi = u[o] >> 16;              // 64 of either stay below 2^32
                for (int d = 32; d > 0; d >>= 1) { lo += __shfl_xor(lo, d); hi += __shfl_xor(hi, d); }
                if ((t & 63) == 0 && (i >> 6) < ACL_FINE) s_sum[o][i >> 6] = ((unsigned long long)hi << 16) + lo;
            }
        }
        __syncthreads();
        // the estimate of every (order, p)
        if (t < 35) {
            const int o = t / 7, p = t % 7;
            long long est = 0x7FFFFFFFFFFFFFFFLL;
            if (o <= maxo && p <= g.pmax) {
                est = (long long)o * bps + 4LL * (1 << p);
                const int per = nfine >> p;                                  // runs per partition (p == 0 for a short block: all)
                for (int q = 0; q < (1 << p); ++q) {
                    long long S = 0;
                    for (int f = q * per; f < (q + 1) * per; ++f) S += (long long)s_sum[o][f];
                    const long long n = (bs >> p) - (q == 0 ? o : 0);
                    const int k = acl_rice_k(n, S);
                    est += n * (k + 1) + (S >> k);
                }
            }
            s_est[t] = est;
        }
        __syncthreads();
        if (t == 0) {
            int best = 0;
            for (int j = 1; j < 35; ++j) if (s_est[j] < s_est[best]) best = j;      // order-major, p-minor: ties to the earlier
            s_pick[0] = best / 7;
            s_pick[1] = best % 7;
        }
        __syncthreads();
        const int o = s_pick[0], p = s_pick[1];
        int big = 0;
        if (t < (1 << p)) {
            const int per = nfine >> p;
            long long S = 0;
            for (int f = t * per; f < (t + 1) * per; ++f) S += (long long)s_sum[o][f];
            const int k = acl_rice_k((bs >> p) - (t == 0 ? o : 0), S);
            s_k[t] = k;
            big = k > 14;
        }
        const int method = __syncthreads_or(big) ? 1 : 0;
        // the winner's exact bits
        const int psize = bs >> p;
        int mine = 0;
        for (int i = t; i < bs; i += 256) {
            if (i < o) continue;
            const int a0 = acl_signal(sL, sR, c, i);
            int r = a0;
            if (o == 1) r = a0 - acl_signal(sL, sR, c, i - 1);
            else if (o == 2) r = a0 - 2 * acl_signal(sL, sR, c, i - 1) + acl_signal(sL, sR, c, i - 2);
            else if (o == 3) r = a0 - 3 * acl_signal(sL, sR, c, i - 1) + 3 * acl_signal(sL, sR, c, i - 2) - acl_signal(sL, sR, c, i - 3);
            else if (o == 4) r = a0 - 4 * acl_signal(sL, sR, c, i - 1) + 6 * acl_signal(sL, sR, c, i - 2) - 4 * acl_signal(sL, sR, c, i - 3) + acl_signal(sL, sR, c, i - 4);
            const int k = s_k[i / psize];
            mine += (int)(acl_fold(r) >> k) + 1 + k;
        }
        const int coded = acl_block_sum_i32(mine, s_red);
        const int exact = 8 + o * bps + 6 + (4 + method) * (1 << p) + coded;
        const int verbatim = 8 + bps * bs;
        if (t == 0) {
            if (exact >= verbatim) { s_rec[c][0] = ACL_T_VERBATIM; s_bits[c] = verbatim; }
            else { s_rec[c][0] = ACL_T_FIXED; s_rec[c][1] = o; s_rec[c][2] = p; s_rec[c][3] = method; s_bits[c] = exact; }
        }
        if (exact < verbatim && t < (1 << p)) s_rec[c][8 + t] = s_k[t];
        __syncthreads();                                    // s_k, s_sum and s_est are free again
    }
    __syncthreads();
    if (t == 0) {
        int code = 0, a = 0, b = -1, total = s_bits[0];
        if (channels == 2) {
            code = 1; a = 0; b = 1; total = s_bits[0] + s_bits[1];
            if (s_bits[0] + s_bits[3] < total) { code = 8; a = 0; b = 3; total = s_bits[0] + s_bits[3]; }
            if (s_bits[3] + s_bits[1] < total) { code = 9; a = 3; b = 1; total = s_bits[3] + s_bits[1]; }
            if (s_bits[2] + s_bits[3] < total) { code = 10; a = 2; b = 3; total = s_bits[2] + s_bits[3]; }
        }
        s_choice[0] = code; s_choice[1] = a; s_choice[2] = b;
        s_choice[3] = acl_header_bytes(g.frame_no, bs, block_size) + (total + 7) / 8 + 2;
        lengths[row] = s_choice[3];
    }
    __syncthreads();
    if (t < ACL_RECORD_INTS) {
        int v = 0;
        if (t == 0) v = s_choice[0];
        else if (t == 1) v = s_choice[3];
        else if (t >= ACL_SUB && t < ACL_SUB + ACL_SUB_INTS) v = s_rec[s_choice[1]][t - ACL_SUB];
        else if (t >= ACL_SUB + ACL_SUB_INTS && t < ACL_SUB + 2 * ACL_SUB_INTS && s_choice[2] >= 0) v = s_rec[s_choice[2]][t - ACL_SUB - ACL_SUB_INTS];
        rec[t] = v;
    }
}

// ---- write --------------------------------------------------------------------------------------------------------------------
// The bit buffer holds the frame MSB-first in 32-bit words: bit b of the frame is bit 31 - (b & 31) of word b >> 5.  Codes that share
// a word go in with LDS atomic OR; a code that would leave the buffer is dropped (the frame is then not copied out: its length is off).
__device__ inline void acl_put(unsigned* buf, int pos, int n, unsigned value) {
    if (n <= 0 || pos < 0 || pos + n > ACL_BUF_WORDS * 32) return;
    if (n < 32) value &= (1u << n) - 1u;
    const int w = pos >> 5, off = pos & 31;
    if (off + n <= 32) {
        atomicOr(&buf[w], value << (32 - off - n));
    } else {
        const int second = off + n - 32;
        atomicOr(&buf[w], value >> second);
        atomicOr(&buf[w + 1], value << (32 - second));
    }
}

__device__ inline unsigned acl_byte(const unsigned* buf, int q) { return (buf[q >> 2] >> (24 - 8 * (q & 3))) & 0xFFu; }

__device__ inline unsigned acl_gf16_mul(unsigned a, unsigned b) {       // a * b mod x^16 + x^15 + x^2 + 1
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

struct acl_sub {
    int type, order, p, method, bps, cand;
};

// bits of item i of a subframe (its sample, with whatever header stands in front of it), written at `pos` when `emit`
__device__ inline int acl_item(unsigned* buf, const int* sig, const acl_sub& s, const int* k_of, int bs, int i, int pos, bool emit) {
    int n = 0;
    if (i == 0) {
        const unsigned head = s.type == ACL_T_VERBATIM ? 2u : s.type == ACL_T_FIXED ? (unsigned)((8 | s.order) << 1) : 0u;
        if (emit) acl_put(buf, pos, 8, head);
        n = 8;
    }
    if (s.type != ACL_T_FIXED || i < s.order) {
        if (emit) acl_put(buf, pos + n, s.bps, (unsigned)sig[i]);
        return n + s.bps;
    }
    const int psize = bs >> s.p, pbits = 4 + s.method;
    if (i == s.order) {
        if (emit) acl_put(buf, pos + n, 6, (unsigned)((s.method << 4) | s.p));
        n += 6;
    }
    const int part = i / psize;
    const int k = k_of[part];
    if (i == s.order || i == part * psize) {
        if (emit) acl_put(buf, pos + n, pbits, (unsigned)k);
        n += pbits;
    }
    int r = sig[i];
    if (s.order == 1) r = sig[i] - sig[i - 1];
    else if (s.order == 2) r = sig[i] - 2 * sig[i - 1] + sig[i - 2];
    else if (s.order == 3) r = sig[i] - 3 * sig[i - 1] + 3 * sig[i - 2] - sig[i - 3];
    else if (s.order == 4) r = sig[i] - 4 * sig[i - 1] + 6 * sig[i - 2] - 4 * sig[i - 3] + sig[i - 4];
    const unsigned u = acl_fold(r);
    const int q = (int)(u >> k);
    if (emit) acl_put(buf, pos + n + q, k + 1, (1u << k) | (u & ((1u << k) - 1u)));      // the unary zeros are there already
    return n + q + 1 + k;
}

__global__ __launch_bounds__(256) void k_flac_write(const unsigned char* __restrict__ pcm, int64_t n_frames, int channels, int width,
                                                    const int64_t* __restrict__ table, int block_size, int rate_code,
                                                    const int* __restrict__ records, const int64_t* __restrict__ offsets,
                                                    unsigned char* __restrict__ out, int64_t total_bytes) {
    __shared__ int sA[ACL_MAX_BLOCK], sB[ACL_MAX_BLOCK];
    __shared__ unsigned s_buf[ACL_BUF_WORDS];
    __shared__ int s_k[2][ACL_FINE];
    __shared__ int s_wave[4];
    __shared__ unsigned s_crc[256];
    const int row = blockIdx.x, t = threadIdx.x;
    const acl_geo g = acl_geometry(table, row, n_frames, block_size);
    if (g.bs == 0) return;
    const int bs = g.bs, bits = 8 * width;
    const int* rec = records + (int64_t)row * ACL_RECORD_INTS;
    // the record, every field inside its range
    int code = rec[0];
    if (channels == 1) code = 0;
    else if (code != 8 && code != 9 && code != 10) code = 1;
    const int promised = rec[1];
    acl_sub sub[2];
    for (int s = 0; s < channels; ++s) {
        const int* r = rec + ACL_SUB + s * ACL_SUB_INTS;
        int type = r[0], order = r[1], p = r[2];
        type = type == ACL_T_CONST || type == ACL_T_FIXED ? type : ACL_T_VERBATIM;
        order = order < 0 ? 0 : (order > 4 ? 4 : order);
        if (order > bs - 1) order = bs - 1;
        p = p < 0 ? 0 : (p > g.pmax ? g.pmax : p);
        sub[s].type = type; sub[s].order = order; sub[s].p = p; sub[s].method = r[3] ? 1 : 0;
        sub[s].cand = channels == 1 ? 0 : (s == 0 ? (code == 9 ? 3 : code == 10 ? 2 : 0) : (code == 1 || code == 9 ? 1 : 3));
        sub[s].bps = bits + (sub[s].cand == 3 ? 1 : 0);
        if (t < ACL_FINE) {
            int k = r[8 + t];
            k = k < 0 ? 0 : (k > (sub[s].method ? 30 : 14) ? (sub[s].method ? 30 : 14) : k);
            s_k[s][t] = k;
        }
    }
    acl_load_words(pcm, g, channels, width, sA, sB);
    for (int j = t; j < ACL_BUF_WORDS; j += 256) s_buf[j] = 0u;
    __syncthreads();
    if (channels == 2) {                                    // the two coded signals in place of L and R: each thread its own samples
        for (int i = t; i < bs; i += 256) {
            const int a = acl_signal(sA, sB, sub[0].cand, i), b = acl_signal(sA, sB, sub[1].cand, i);
            sA[i] = a; sB[i] = b;
        }
    }
    __syncthreads();                                        // a residual reads the four samples in front of its own
    // the header, by one thread; the bytes land in words of their own, so plain ORs into the zeroed buffer
    const int hbytes = acl_header_bytes(g.frame_no, bs, block_size);
    if (t == 0) {
        unsigned char h[12];
        int n = 0;
        int size_code = 6;
        if (bs == block_size) { size_code = 8; for (int v = block_size; v > 256; v >>= 1) ++size_code; }
        else if (bs - 1 >= 256) size_code = 7;
        h[n++] = 0xFF; h[n++] = 0xF8;
        h[n++] = (unsigned char)((size_code << 4) | (rate_code & 15));
        h[n++] = (unsigned char)((code << 4) | ((width == 2 ? 4 : 6) << 1));
        const int f = g.frame_no;
        if (f < 128) h[n++] = (unsigned char)f;
        else if (f < 2048) { h[n++] = (unsigned char)(0xC0 | (f >> 6)); h[n++] = (unsigned char)(0x80 | (f & 63)); }
        else if (f < 65536) { h[n++] = (unsigned char)(0xE0 | (f >> 12)); h[n++] = (unsigned char)(0x80 | ((f >> 6) & 63)); h[n++] = (unsigned char)(0x80 | (f & 63)); }
        else { h[n++] = (unsigned char)(0xF0 | (f >> 18)); h[n++] = (unsigned char)(0x80 | ((f >> 12) & 63)); h[n++] = (unsigned char)(0x80 | ((f >> 6) & 63)); h[n++] = (unsigned char)(0x80 | (f & 63)); }
        if (size_code == 6) h[n++] = (unsigned char)(bs - 1);
        else if (size_code == 7) { h[n++] = (unsigned char)((bs - 1) >> 8); h[n++] = (unsigned char)((bs - 1) & 255); }
        unsigned c8 = 0;
        for (int j = 0; j < n; ++j) {
            c8 ^= h[j];
            for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
        }
        h[n++] = (unsigned char)c8;
        for (int j = 0; j < n; ++j) acl_put(s_buf, 8 * j, 8, h[j]);
    }
    // the subframes: a thread owns a run of consecutive samples, counts its bits, takes its place from a scan and writes
    const int per = (bs + 255) / 256;
    const int i_lo = t * per < bs ? t * per : bs, i_hi = (t + 1) * per < bs ? (t + 1) * per : bs;
    int pos = 8 * hbytes;
    for (int s = 0; s < channels; ++s) {
        const int* sig = s == 0 ? sA : sB;
        int total;
        if (sub[s].type == ACL_T_CONST) {
            if (t == 0) { acl_put(s_buf, pos, 8, 0u); acl_put(s_buf, pos + 8, sub[s].bps, (unsigned)sig[0]); }
            total = 8 + sub[s].bps;
        } else {
            int mine = 0;
            for (int i = i_lo; i < i_hi; ++i) mine += acl_item(s_buf, sig, sub[s], s_k[s], bs, i, 0, false);
            int incl = mine;                                // inclusive scan across the wave, then across the four waves
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if ((t & 63) >= d) incl += up;
            }
            __syncthreads();                                // s_wave of the subframe before
            if ((t & 63) == 63) s_wave[t >> 6] = incl;
            __syncthreads();
            int before = 0;
            for (int w = 0; w < (t >> 6); ++w) before += s_wave[w];
            total = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
            int at = pos + before + incl - mine;
            for (int i = i_lo; i < i_hi; ++i) at += acl_item(s_buf, sig, sub[s], s_k[s], bs, i, at, true);
        }
        pos += total;
    }
    const int body_end = (pos + 7) / 8;                     // the zero padding is there already
    const int flen = body_end + 2;
    __syncthreads();
    // CRC-16 of bytes [0, body_end): per-thread CRCs of equal chunks aligned to the end, combined pairwise by x^(8 * chunk * 2^level)
    const bool fits = flen <= ACL_BUF_WORDS * 4 && pos <= ACL_BUF_WORDS * 32;
    const int n_crc = fits ? body_end : 0;
    const int chunk = (n_crc + 255) / 256;
    {
        const int end = n_crc - (255 - t) * chunk;
        const int begin = end - chunk < 0 ? 0 : end - chunk;
        unsigned c = 0;
        for (int q = begin; q < end; ++q) {
            c ^= acl_byte(s_buf, q) << 8;
            for (int b = 0; b < 8; ++b) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        }
        s_crc[t] = c;
        unsigned m = 1;                                     // x^(8 * chunk)
        for (int j = 0; j < 8 * chunk; ++j) { m <<= 1; if (m & 0x10000u) m ^= 0x18005u; }
        for (int step = 1; step < 256; step <<= 1) {
            __syncthreads();
            unsigned mixed = 0;
            const bool right = (t & (2 * step - 1)) == 2 * step - 1;
            if (right) mixed = acl_gf16_mul(s_crc[t - step], m) ^ s_crc[t];
            __syncthreads();
            if (right) s_crc[t] = mixed;
            m = acl_gf16_mul(m, m);
        }
        __syncthreads();
    }
    if (t == 0 && fits) acl_put(s_buf, 8 * body_end, 16, s_crc[255]);
    __syncthreads();
    // out: whole dwords where the address is aligned, bytes at the two ends; only a frame that is what its record promised
    const int64_t off = offsets[row];
    if (!fits || flen != promised || off < 0 || off > total_bytes - flen) return;
    unsigned char* dst = out + off;
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > flen) head = flen;
    const int n_dw = (flen - head) / 4, tail = flen - head - 4 * n_dw;
    if (t < head) dst[t] = (unsigned char)acl_byte(s_buf, t);
    for (int j = t; j < n_dw; j += 256) {
        const int q = head + 4 * j;
        const unsigned v = acl_byte(s_buf, q) | (acl_byte(s_buf, q + 1) << 8) | (acl_byte(s_buf, q + 2) << 16) | (acl_byte(s_buf, q + 3) << 24);
        *reinterpret_cast<unsigned*>(dst + q) = v;
    }
    if (t < tail) dst[head + 4 * n_dw + t] = (unsigned char)acl_byte(s_buf, head + 4 * n_dw + t);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
static int acl_check_common(const void* pcm, int64_t n_frames, int channels, int width, const void* table, int n_table, int block_size) {
    ACL_REQUIRE(pcm && table, "null pointer");
    ACL_REQUIRE(n_frames > 0 && n_frames < (1LL << 40), "n_frames must be in (0, 2^40)");
    ACL_REQUIRE(channels == 1 || channels == 2, "channels must be 1 or 2");
    ACL_REQUIRE(width == 2 || width == 3, "width must be 2 (PCM_16) or 3 (PCM_24)");
    ACL_REQUIRE(n_table > 0, "n_table must be positive");
    ACL_REQUIRE(block_size == 256 || block_size == 512 || block_size == 1024 || block_size == 2048 || block_size == 4096,
                "block_size must be 256, 512, 1024, 2048 or 4096");
    ACL_REQUIRE((((uintptr_t)table) & 7) == 0, "table must be 8-byte aligned");
    return AC_OK;
}

extern "C" int acl_flac_plan(const unsigned char* pcm, int64_t n_frames, int channels, int width, const int64_t* table, int n_table,
                             int block_size, int* records, int* lengths, void* stream) {
    if (int rc = acl_check_common(pcm, n_frames, channels, width, table, n_table, block_size)) return rc;
    ACL_REQUIRE(records && lengths, "null pointer");
    ACL_REQUIRE((((uintptr_t)records) & 3) == 0 && (((uintptr_t)lengths) & 3) == 0, "records and lengths must be 4-byte aligned");
    hipLaunchKernelGGL(k_flac_plan, dim3((unsigned)n_table), dim3(256), 0, (hipStream_t)stream, pcm, n_frames, channels, width, table,
                       block_size, records, lengths);
    ACL_LAUNCH_CHECK();
    return AC_OK;
}

extern "C" int acl_flac_write(const unsigned char* pcm, int64_t n_frames, int channels, int width, const int64_t* table, int n_table,
                              int block_size, int rate_code, const int* records, const int64_t* offsets, unsigned char* out,
                              int64_t total_bytes, void* stream) {
    if (int rc = acl_check_common(pcm, n_frames, channels, width, table, n_table, block_size)) return rc;
    ACL_REQUIRE(records && offsets && out, "null pointer");
    ACL_REQUIRE(rate_code >= 0 && rate_code <= 11, "rate_code must be in [0, 11]");
    ACL_REQUIRE(total_bytes > 0, "total_bytes must be positive");
    ACL_REQUIRE((((uintptr_t)records) & 3) == 0 && (((uintptr_t)offsets) & 7) == 0, "records and offsets must be aligned to their words");
    hipLaunchKernelGGL(k_flac_write, dim3((unsigned)n_table), dim3(256), 0, (hipStream_t)stream, pcm, n_frames, channels, width, table,
                       block_size, rate_code, records, offsets, out, total_bytes);
    ACL_LAUNCH_CHECK();
    return AC_OK;
}
