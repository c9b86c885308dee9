// The `vocal_separation` mode's 24-bit stem writer (include/audiocut_hip_export.h): iSTFT waves + resident track -> the two stems
// as finished 24-bit PCM and the three energy sums of the confidence estimate, in one pass.  The kernel is k_mdx_assemble_pcm
// (ac_pack.hip), which is templated on the subtype of the word it stores; this entry point is its AC_PACK_PCM_24 instance - the
// checks (an output stream of 24-bit words needs 4-byte alignment), the launch and every byte are those of ac_mdx_assemble_pcm.
#include "ac_common.h"
#include "../../include/audiocut_hip_export.h"
#include "../../include/audiocut_hip_pack.h"

extern "C" int ac_export_abi_version(void) { return AC_EXPORT_ABI_VERSION; }

extern "C" int ac_mdx_assemble_pcm24(ac_ctx* ctx, const float* track, int64_t n, int channels, const float* wave,
                                     const int64_t* chunk_start, const int64_t* chunk_len, const int64_t* eff_start,
                                     const int64_t* eff_end, const int32_t* item_base, int n_chunks, unsigned char* stem_out,
                                     unsigned char* rest_out, double* partials, int n_partials, void* stream) {
    return ac_mdx_assemble_pcm(ctx, track, n, channels, wave, chunk_start, chunk_len, eff_start, eff_end, item_base, n_chunks,
                               AC_PACK_PCM_24, stem_out, rest_out, partials, n_partials, stream);
}
