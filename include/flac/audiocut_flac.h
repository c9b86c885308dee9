/*
 * audiocut_flac.h — lossless FLAC frames encoded on the device, from the finished, interleaved, little-endian PCM bytes the
 * packing kernels leave there (ac_pack_pcm, acf_pack_spans, ac_resample_poly_pack, ac_mdx_assemble_pcm).  This is the C ABI of
 * libaudiocut_flac.so (gfx950), a third small library next to libaudiocut_hip.so and libaudiocut_finish.so: it takes no ac_ctx,
 * keeps its own error text (acl_last_error) and shares only the error codes of include/audiocut_hip.h.
 *
 * The host statement of the encoder is `flac_encode_host` (audio_cut_amd/utils/flac_export.py): integer arithmetic only, so
 * these kernels reproduce its bytes.  A file decodes to exactly the integer samples the WAV of the same subtype holds.
 *
 * ---- The stream: RFC 9639's layout restricted to what this encoder emits.  All fields MSB-first, multi-byte fields big-endian. ----
 *
 * File.  `fLaC`; one metadata block header 80 00 00 22 (last-block flag, type 0, length 34); STREAMINFO: minimum and maximum block
 * size (16 bits each, both the configured block size, even when the only or last frame is shorter), minimum and maximum frame size
 * in bytes (24 bits each, the true values of this file), sample rate (20 bits), channels - 1 (3 bits), bits per sample - 1
 * (5 bits), total samples per channel (36 bits), MD5 of the PCM bytes (128 bits; 16 zero bytes = not computed).  Then the frames.
 * A rate above 1 048 575 Hz, or a file of 2^21 or more frames, is refused on the host.  (The 42 bytes are written on the host.)
 *
 * Frame header.  14 bits 11111111111110; one reserved 0 bit; blocking strategy 0 (fixed); block-size code (4 bits): 1000..1100
 * for 256..4096, for a shorter last block 0110 if size - 1 < 256 with size - 1 as 8 bits at the end of the header, otherwise 0111
 * with size - 1 as 16 bits; sample-rate code (4 bits): 88.2k 0001, 176.4k 0010, 192k 0011, 8k 0100, 16k 0101, 22.05k 0110,
 * 24k 0111, 32k 1000, 44.1k 1001, 48k 1010, 96k 1011, any other rate 0000 (see STREAMINFO); channel assignment (4 bits): 0000
 * mono, 0001 L,R independent, 1000 left/side, 1001 side/right, 1010 mid/side; sample size (3 bits): 100 for 16 bits, 110 for 24;
 * one reserved 0 bit; the frame number within the file in the UTF-8-style variable-length code (1 byte below 128, 2 below 2048,
 * 3 below 65 536, 4 below 2^21); the optional block-size bytes; CRC-8 of every header byte before it (polynomial 0x07, initial
 * value 0).
 *
 * Subframe.  One per channel, in assignment order; the side channel carries one bit more than the stream's sample size.  One 0
 * bit; six type bits: 000000 constant, 000001 verbatim, 001ooo fixed predictor of order ooo <= 4; a 0 wasted-bits flag; then
 * constant: the value; verbatim: all samples; fixed: `order` warm-up samples, then the residual.  Side is L - R, mid is
 * (L + R) >> 1 (arithmetic shift).  Fixed residuals are the order-th finite difference, coefficients 1; 1,-1; 1,-2,1; 1,-3,3,-1;
 * 1,-4,6,-4,1: at most 25 + 4 bits, so int32 holds them.
 *
 * Residual.  Two method bits (00: 4-bit Rice parameters, 01: 5-bit); four bits of partition order p; 2^p partitions, the first of
 * (block >> p) - order residuals, the others of block >> p; each a parameter k and its residuals.  A residual r is folded to
 * u = r >= 0 ? 2r : -2r - 1 and written as u >> k zero bits, a one bit, the low k bits of u.  No escape parameter.
 *
 * Frame end.  Zero bits up to a byte boundary, then CRC-16 of the whole frame from the sync code on (polynomial 0x8005, initial
 * value 0, no reflection), high byte first.
 *
 * Known answers: CRC-8 of ASCII 123456789 is 0xF4, CRC-16 is 0xFEE8.  4096 zero samples, mono, 16 bits, 44 100 Hz, block 4096,
 * MD5 unset, are the 53 bytes
 *   66 4c 61 43 80 00 00 22 10 00 10 00 00 00 0b 00 00 0b 0a c4 40 f0 00 00 10 00
 *   00 00 00 00 00 00 00 00 00 00 00 00 00 00 00 00 ff f8 c9 08 00 95 00 00 00 21 bd
 *
 * ---- The choices (flac_export.py states them; every tie goes to the earlier option, the smaller order, p and k) ----
 * Per frame and candidate signal (mono: the channel; stereo: L, R, mid, side): all samples equal -> constant.  Otherwise, for
 * orders 0..min(4, block - 1) and partition orders 0..pmax (pmax = log2(block_size / 64) for a full block, 0 for a shorter last
 * one): per partition of n residuals with S = the sum of u, k = the smallest k with (n << k) >= S; the estimate of (order, p) is
 * order * bps + 4 * 2^p + the sum of n * (k + 1) + (S >> k); the smallest estimate is selected and its bits counted exactly
 * (method 01 if one of its k exceeds 14); verbatim whenever that count is not smaller than 8 + bps * block.  A stereo frame takes
 * the assignment with the fewest exact bits among independent, left/side, side/right, mid/side.
 *
 * ---- The two launches ----
 * Both are driven by a frame table on the device, int64 [n_table][4]: (file index, frame number within the file, first frame of
 * the track, block length).  Neither trusts it: the first frame is clamped to [0, n_frames], the block length to what is left of
 * the track and to block_size, the frame number to 21 bits; a frame whose clamped block is empty produces nothing.  One
 * workgroup of 256 threads per table row.
 *
 * Conventions: those of include/audiocut_hip.h (device pointers, asynchronous on `stream`, 0 = ok, negative = AC_E_INVALID /
 * AC_E_HIP with the text in acl_last_error(), thread-local).
 */
#ifndef AUDIOCUT_FLAC_H
#define AUDIOCUT_FLAC_H

#include "../audiocut_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACL_ABI_VERSION 1

/* int32 words of one frame's record: [0] channel assignment code, [1] the frame's bytes, then per subframe s at 8 + 72 s:
 * [0] type (0 constant, 1 verbatim, 2 fixed), [1] order, [2] p, [3] method, [8..71] k of each partition */
#define ACL_RECORD_INTS 160
/* the largest frame: header 11, two verbatim 24-bit subframes of 4096 samples, CRC-16 */
#define ACL_MAX_FRAME_BYTES 24591

int acl_abi_version(void);
const char* acl_last_error(void);

/* Chooses every frame's coding and counts its bytes exactly: records [n_table][ACL_RECORD_INTS] int32 and lengths [n_table] int32
 * (0 for an empty frame), both written in full.  pcm: n_frames * channels * width bytes; channels 1 or 2, width 2 or 3,
 * block_size 256, 512, 1024, 2048 or 4096, 0 < n_frames < 2^40, n_table > 0. */
int acl_flac_plan(const unsigned char* pcm, int64_t n_frames, int channels, int width, const int64_t* table, int n_table,
                  int block_size, int* records, int* lengths, void* stream);

/* Writes every frame at offsets[row] of out (int64 [n_table], the exclusive scan of the lengths): lengths[row] bytes each,
 * nothing past a frame's own bytes and nothing outside [0, total_bytes); a frame that would not fit there, or whose record does
 * not give the length its bits come to, is not written.  rate_code: the header's 4-bit sample-rate code. */
int acl_flac_write(const unsigned char* pcm, int64_t n_frames, int channels, int width, const int64_t* table, int n_table,
                   int block_size, int rate_code, const int* records, const int64_t* offsets, unsigned char* out,
                   int64_t total_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AUDIOCUT_FLAC_H */
