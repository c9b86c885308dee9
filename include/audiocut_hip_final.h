/*
 * audiocut_hip_final.h — the TFC-TDF U-Net's last TDF layer with the graph's final 1x1 convolution in its epilogue, an extension
 * of the C ABI of libaudiocut_hip.so (gfx950).  The entry points below are exported by the same library as
 * include/audiocut_hip.h, whose declarations, conventions and ABI version (6) they leave unchanged; this header has a version
 * of its own.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, element counts, asynchronous on `stream`, 0 = ok).
 */
#ifndef AUDIOCUT_HIP_FINAL_H
#define AUDIOCUT_HIP_FINAL_H

#include "audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AC_FINAL_ABI_VERSION 1

int ac_final_abi_version(void);

/* Second TDF layer of the last decoder block and the final (C -> C_out) 1x1 convolution, one kernel:
 *   y[m][n]            = resid[m][n] + relu(scale[c] * w_unscale * sum_k x[m][k] w[n][k] + shift[c]),   c = (m / T) % C
 *   spec[b][co][t][n]  = a_C,  a_0 = final_b[co],  a_(c+1) = fmaf(final_w[co][c], y[(b, c, t)][n], a_c)
 * Both results are bit-identical to ac_tdf_linear_f16x3 followed by ac_conv1x1_small without its ReLU on the same operands: every GEMM
 * row is split at its own time row's scale and accumulated in the same order, and the channel sum is the same float32 FMA chain.
 * A workgroup tile is all 48 channels x 2 consecutive time rows x 192 columns, so y never has to exist in memory:
 *   y  NULL: only spec [M / (C * T)][C_out][T][N] is written;   y non-NULL: y [M][N] is stored as well (block taps, tests).
 * x [M][K] float32, resid [M][N] (required), w_packed from conv_pack.pack_linear (its 192-column layout), final_w [C_out][C],
 * final_b [C_out], in_amax [M / (C * T)][T] or NULL as for ac_tdf_linear_f16x3.
 * M = items * C * T with 96 % C == 0 and T % (96 / C) == 0, of which the tile of C = 48 (T % 2 == 0) is the one built;
 * N % 192 == 0, K % 32 == 0, 1 <= C_out <= 4, fewer than 2^31 - 8 workgroups (M / 96 * N / 192).  Any other shape is refused
 * (AC_E_INVALID) before anything is launched. */
int ac_tdf_linear_final_f16x3(ac_ctx* ctx, const float* x, const void* w_packed, const float* scale, const float* shift,
                              const float* resid, const float* final_w, const float* final_b, float* spec, float* y,
                              long long M, int N, int K, int T, int C, int C_out, float w_unscale, const float* in_amax,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_HIP_FINAL_H */
