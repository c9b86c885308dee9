// Device side of the float64 STFT-2048 shared by ac_frames.hip (flatness / mel, centroid + low-third ratio) and ac_beat.hip
// (centroid + bandwidth): one 256-thread workgroup per frame, the real FFT through a 1024-point complex radix-4 Stockham FFT in LDS.
// librosa.stft multiplies the float64 periodic Hann into the frames before the FFT and only then rounds to complex64; every
// helper below keeps that order, and every kernel that calls one forms the same values with the same operations in the same order.
#pragma once
#include <math.h>

#include "ac_common.h"

__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// 1024-point complex forward FFT, 256 threads, 5 radix-4 Stockham passes; result in `a` (ping-pong with `b`).
__device__ inline double2* fft1024_f64(double2* a, double2* b, const double2* __restrict__ tw2048) {
    const int j = threadIdx.x;            // butterfly index, 0..255
    int Ns = 1;
#pragma unroll
    for (int pass = 0; pass < 5; ++pass) {
        const int k = j & (Ns - 1);
        double2 v0 = a[j], v1 = a[j + 256], v2 = a[j + 512], v3 = a[j + 768];
        // twiddle exp(-2*pi*i*k*m/(4*Ns)) = tw2048[k*m*(2048/(4*Ns))]
        const int stride = 512 / Ns;      // 2048 / (4*Ns)
        if (Ns > 1) {
            v1 = cmul(v1, tw2048[k * stride]);
            const int i2 = 2 * k * stride, i3 = 3 * k * stride;   // < 2048*3/4 ; tw table holds k < 1024: fold
            double2 t2 = tw2048[i2 & 1023]; if (i2 & 1024) { t2.x = -t2.x; t2.y = -t2.y; }
            double2 t3 = tw2048[i3 & 1023]; if (i3 & 1024) { t3.x = -t3.x; t3.y = -t3.y; }
            v2 = cmul(v2, t2);
            v3 = cmul(v3, t3);
        }
        // radix-4 butterfly (forward: -i rotation)
        const double2 s02 = make_double2(v0.x + v2.x, v0.y + v2.y), d02 = make_double2(v0.x - v2.x, v0.y - v2.y);
        const double2 s13 = make_double2(v1.x + v3.x, v1.y + v3.y), d13 = make_double2(v1.x - v3.x, v1.y - v3.y);
        const int base = ((j - k) << 2) + k;
        b[base] = make_double2(s02.x + s13.x, s02.y + s13.y);
        b[base + Ns] = make_double2(d02.x + d13.y, d02.y - d13.x);
        b[base + 2 * Ns] = make_double2(s02.x - s13.x, s02.y - s13.y);
        b[base + 3 * Ns] = make_double2(d02.x - d13.y, d02.y + d13.x);
        __syncthreads();
        double2* t = a; a = b; b = t;
        Ns <<= 2;
    }
    return a;
}

// The windowed frame of 2048 samples from s0 on, packed for the real FFT: z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1].  Samples
// outside [lo, hi) read as zero (the centred frame's zero padding).  Ends with a barrier: s_a is complete on return.
__device__ inline void stft2048_load_frame(const float* __restrict__ x, int64_t s0, int64_t lo, int64_t hi,
                                           const double* __restrict__ hann, double2* s_a) {
    for (int m = threadIdx.x; m < 1024; m += 256) {
        const int64_t g0 = s0 + 2 * m, g1 = g0 + 1;
        const double a0 = (g0 >= lo && g0 < hi) ? (double)x[g0] : 0.0;
        const double a1 = (g1 >= lo && g1 < hi) ? (double)x[g1] : 0.0;
        s_a[m] = make_double2(a0 * hann[2 * m], a1 * hann[2 * m + 1]);
    }
    __syncthreads();
}

// Bin k (0..1024) of the 2048-point real spectrum from the packed transform Z, as librosa stores it: complex64.
// untangle: X[k] = (Z[k] + conj(Z[N-k]))/2 - i W^k (Z[k] - conj(Z[N-k]))/2, N = 1024, W = exp(-2 pi i/2048)
__device__ inline float2 stft2048_bin_c64(const double2* Z, const double2* __restrict__ tw, int k) {
    const double2 zk = Z[k & 1023];
    const double2 zn = Z[(1024 - k) & 1023];
    const double2 e = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
    const double2 o = make_double2(0.5 * (zk.x - zn.x), 0.5 * (zk.y + zn.y));
    double2 w = (k < 1024) ? tw[k] : make_double2(-1.0, 0.0);
    // -i * w * o
    const double2 wo = cmul(w, o);
    return make_float2((float)(e.x + wo.y), (float)(e.y - wo.x));
}

// np.abs of the complex64 bin: float32
__device__ inline float stft2048_mag_f32(float2 c) { return (float)sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y); }

// s_m[k] = |X[k]| for the 1025 bins of the frame held in Z.  Ends with a barrier.
__device__ inline void stft2048_magnitudes(const double2* Z, const double2* __restrict__ tw, float* s_m) {
    for (int k = threadIdx.x; k <= 1024; k += 256) s_m[k] = stft2048_mag_f32(stft2048_bin_c64(Z, tw, k));
    __syncthreads();
}

// librosa.util.normalize(S, norm=1, axis=-2) of one column: the length is measured in float64, a length under float32's
// tiny becomes 1, and S / length goes back to float32.
__device__ inline float stft2048_norm1(float s, double len_eff) { return (float)((double)s / len_eff); }

// librosa.feature.spectral_centroid of the column in s_m (1025 float32 magnitudes in LDS): sum_k f_k * norm1(S_k), f_k = k sr / 2048.
// Two strided sweeps and three block reductions in a fixed order; s_red holds 12 doubles.  *length = sum of the magnitudes,
// *lowsum = sum over the low third (k < 1025 / 3), *len_eff = the divisor `normalize` uses.  Every thread gets every value.
__device__ inline double stft2048_centroid(const float* s_m, double sr, double* s_red, double* length, double* lowsum, double* len_eff) {
    double tot = 0.0, low = 0.0;
    for (int k = threadIdx.x; k <= 1024; k += 256) { const double v = (double)s_m[k]; tot += v; if (k < 1025 / 3) low += v; }
    *length = block_sum_f64_256(tot, s_red);
    *lowsum = block_sum_f64_256(low, s_red + 4);
    *len_eff = *length < 1.17549435e-38 ? 1.0 : *length;
    double c = 0.0;
    for (int k = threadIdx.x; k <= 1024; k += 256) {
        const float sn = stft2048_norm1(s_m[k], *len_eff);
        c += ((double)k * sr / 2048.0) * (double)sn;
    }
    return block_sum_f64_256(c, s_red + 8);
}
