"""The C ABI of libaudiocut_hip.so, header by header: what include/*.h declares, what `_native.ABI_SURFACES` binds, what the
library exports and the table below are one surface - the same names, the same version, the same types in the same order - and
every export names the GPU test that calls it directly.  A new entry point or header fails here until its row is written.  CPU only."""
import ast
import functools
import re

import pytest

import abi_surface as A
from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd import _native

N_EXPORTS, N_MAIN_EXPORTS = 78, 49

# header -> (its version function, its version, {every export -> the GPU test that calls it directly and compares it with a
# reference ("module::test"), or "host-only": versions, context and error plumbing, size queries, the host C++ beat DP})
SURFACES = {
    "audiocut_hip.h": ("ac_abi_version", 6, {
        "ac_abi_version": "host-only",
        "ac_last_error": "host-only",
        "ac_ctx_create": "host-only",
        "ac_ctx_destroy": "host-only",
        "ac_next_leq_scratch": "host-only",
        "ac_tempogram_parts": "host-only",
        "ac_local_valley_tiles": "host-only",
        "ac_host_beat_dp": "host-only",
        "ac_frame_rms": "test_kernels_gpu::test_frame_rms",
        "ac_frame_rms_multi": "test_kernels_gpu::test_frame_rms_multi_is_the_single_kernel_bit_for_bit",
        "ac_stft2048_features": "test_kernels_gpu::test_stft_flatness_and_mel",
        "ac_onset_strength": "test_kernels_gpu::test_onset_strength",
        "ac_tempogram_reduce": "test_kernels_gpu::test_tempogram_reduce",
        "ac_yin_f0": "test_kernels_gpu::test_yin_f0_autocorrelation_kernel",
        "ac_moving_meansq_db_f64": "test_cut_refine_edges_gpu::test_moving_meansq_db_edges",
        "ac_next_leq_scan": "test_cut_refine_edges_gpu::test_next_leq_scan_edges",
        "ac_window_argmin_f64": "test_cut_refine_edges_gpu::test_window_argmin_edges",
        "ac_zero_cross_nearest": "test_cut_refine_edges_gpu::test_zero_cross_nearest_edges",
        "ac_quiet_guard_slow": "test_cut_refine_edges_gpu::test_quiet_guard_slow_edges",
        "ac_pause_cut_points": "test_cut_refine_edges_gpu::test_pause_cut_points_edges",
        "ac_mdx_stft": "test_mdx_kernels_gpu::test_stft_against_float64",
        "ac_mdx_istft": "test_mdx_kernels_gpu::test_istft_against_float64",
        "ac_mdx_assemble_ola": "test_mdx_kernels_gpu::test_assemble_ola_exact_over_plans",
        "ac_mdx_chunk_vocal": "test_kernels_edges_gpu::test_mdx_chunk_vocal_edges",
        "ac_sum_squares": "test_kernels_edges_gpu::test_mean_square_partials_edges",
        "ac_window_sum_squares": "test_kernels_gpu::test_window_mean_squares_is_the_per_window_mean_square_bit_for_bit",
        "ac_conv3x3_f16x3": "test_unet_gpu::test_conv3x3_f16x3_kernel",
        "ac_conv3x3_f16x3_w96": "test_unet_gpu::test_conv3x3_f16x3_w96_kernel",
        "ac_conv3x3_f16x3_s8": "test_kernels_edges_gpu::test_level0_conv_at_64_items_matches_2_items",
        "ac_conv3x3_f16x3_first": "test_unet_gpu::test_first_conv_fused_into_the_3x3_loader_is_bit_identical",
        "ac_conv1x1_small": "test_unet_gpu::test_conv1x1_small_kernel",
        "ac_tdf_linear_f16x3": "test_unet_gpu::test_tdf_linear_f16x3_kernel",
        "ac_tdf_small_fused": "test_unet_gpu::test_tdf_small_fused_kernel",
        "ac_down2x_f16x3": "test_unet_gpu::test_fused_resampling_kernels_vs_float64",
        "ac_up2x_f16x3": "test_unet_gpu::test_fused_resampling_kernels_vs_float64",
        "ac_pyin_observe": "test_pitch_kernels_gpu::test_observe_crafted_rows",
        "ac_pyin_viterbi": "test_pitch_kernels_gpu::test_viterbi_bit_exact",
        "ac_lpc_formants": "test_pitch_kernels_gpu::test_lpc_formants_exact",
        "ac_zero_crossing_rate": "test_kernels_edges_gpu::test_zero_crossing_rate_edges",
        "ac_stft2048_spectral": "test_kernels_edges_gpu::test_stft2048_spectral_edges",
        "ac_segment_frame_rms": "test_kernels_edges_gpu::test_segment_frame_rms_edges",
        "ac_segment_sumsq_peak": "test_kernels_edges_gpu::test_segment_sumsq_peak_edges",
        "ac_local_valley": "test_kernels_edges_gpu::test_local_valley_edges",
        "ac_resample_poly": "test_resample_pcm_edges_gpu::test_resample_poly_same_taps",
        "ac_resample_poly_segments": "test_kernels_edges_gpu::test_resample_poly_segments_edges",
        "ac_pack_pcm24": "test_resample_pcm_edges_gpu::test_pack_pcm24_known_answers_in_every_lane_and_in_the_tail",
        "ac_silero_frontend": "test_silero_kernels_gpu::test_frontend_against_float64",
        "ac_silero_lstm": "test_silero_kernels_gpu::test_lstm_synthetic_gates",
        "ac_silero_out": "test_silero_kernels_gpu::test_out_against_float64",
    }),
    "audiocut_hip_stereo.h": ("ac_stereo_abi_version", 1, {
        "ac_stereo_abi_version": "host-only",
        "ac_mdx_stft_stereo": "test_mdx_kernels_gpu::test_stft_against_float64",
        "ac_mdx_assemble_ola_stereo": "test_mdx_kernels_gpu::test_assemble_ola_exact_over_plans",
        "ac_mdx_chunk_vocal_stereo": "test_stereo_kernels_gpu::test_mdx_chunk_vocal_stereo_exact",
    }),
    "audiocut_hip_onset.h": ("ac_onset_abi_version", 1, {
        "ac_onset_abi_version": "host-only",
        "ac_bar_energy_silence": "test_smart_segment_gpu::test_bar_energy_silence_against_numpy",
        "ac_segment_pair_energy": "test_smart_segment_gpu::test_segment_pair_energy_against_numpy",
    }),
    "audiocut_hip_beat.h": ("ac_beat_abi_version", 1, {
        "ac_beat_abi_version": "host-only",
        "ac_stft2048_centroid_bandwidth": "test_beat_analysis_gpu::test_centroid_bandwidth_against_librosa",
        "ac_bar_means3": "test_beat_analysis_gpu::test_bar_means3_against_numpy",
    }),
    "audiocut_hip_hybrid.h": ("ac_hybrid_abi_version", 1, {
        "ac_hybrid_abi_version": "host-only",
        "ac_quiet_gate_meansq": "test_hybrid_gpu::test_quiet_gate_meansq_against_numpy",
    }),
    "audiocut_hip_export.h": ("ac_export_abi_version", 1, {
        "ac_export_abi_version": "host-only",
        "ac_mdx_assemble_pcm24": "test_vocal_separation_gpu::test_assemble_pcm24_exact_over_plans",
    }),
    "audiocut_hip_asr.h": ("ac_asr_abi_version", 1, {
        "ac_asr_abi_version": "host-only",
        "ac_resample_poly_pcm16": "test_vpbd_asr_gpu::test_pcm16_kernel_is_the_float_kernel_through_the_host_conversion",
    }),
    "audiocut_hip_profile.h": ("ac_profile_abi_version", 1, {
        "ac_profile_abi_version": "host-only",
        "ac_abs_peak_coverage": "test_auto_profile_gpu::test_coverage_kernel_exact",
    }),
    "audiocut_hip_final.h": ("ac_final_abi_version", 1, {
        "ac_final_abi_version": "host-only",
        "ac_tdf_linear_final_f16x3": "test_tdf_final_fused_gpu::test_fused_final_is_the_two_kernels_bit_for_bit",
    }),
    "audiocut_hip_load.h": ("ac_load_abi_version", 1, {
        "ac_load_abi_version": "host-only",
        "ac_decode_pcm": "test_wav_decode_gpu::test_decode_matches_decode_host",
    }),
    "audiocut_hip_pack.h": ("ac_pack_abi_version", 1, {
        "ac_pack_abi_version": "host-only",
        "ac_pack_width": "host-only",
        "ac_pack_out_align": "host-only",
        "ac_pack_pcm": "test_export_subtypes_gpu::test_pack_pcm_against_the_host_conversion",
        "ac_mdx_assemble_pcm": "test_export_subtypes_gpu::test_assemble_pcm_against_assemble_then_pack",
    }),
    "audiocut_hip_rate.h": ("ac_rate_abi_version", 1, {
        "ac_rate_abi_version": "host-only",
        "ac_resample_poly_pack": "test_output_rate_gpu::test_kernel_is_the_composition_and_the_host_statement",
    }),
}


@functools.lru_cache(maxsize=None)
def _top_level_functions(module: str) -> set:
    tree = ast.parse((A.ROOT / "tests" / f"{module}.py").read_text())
    return {node.name for node in tree.body if isinstance(node, ast.FunctionDef)}


@pytest.mark.parametrize("header", list(SURFACES))
def test_header_registry_library_and_table_are_one_surface(lib, header):
    version_fn, version, export_tests = SURFACES[header]
    surface = {s.header: s for s in _native.ABI_SURFACES}[header]
    protos = A.prototypes(header)
    names = [name for _, name, _ in protos]
    assert len(set(names)) == len(names), f"{header} declares a name twice"
    assert set(names) == set(surface.signatures) == set(export_tests)
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in {header} but the library does not export it"
    assert version_fn in names and surface.version_fn == version_fn
    assert A.defined_version(header, version_fn) == surface.version == version == getattr(lib, version_fn)()
    # every prototype, type by type, against the ctypes signature: the same ctypes objects in the same order
    for c_res, name, c_params in protos:
        restype, argtypes = surface.signatures[name]
        assert restype is A.ctype(c_res, is_return=True), f"{name}: returns {c_res}, bound as {restype.__name__}"
        want = [A.ctype(p) for p in c_params]
        assert len(argtypes) == len(want), f"{name}: {len(want)} parameters in {header}, {len(argtypes)} argtypes"
        for i, (got, exp) in enumerate(zip(argtypes, want)):
            assert got is exp, f"{name}: parameter {i} is {c_params[i]} in {header}, bound as {got.__name__}"
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == list(argtypes)
    # every export names the GPU test that calls it directly, and that test exists
    for name, ref in export_tests.items():
        if ref != "host-only":
            module, test = ref.split("::")
            assert test in _top_level_functions(module), f"{name}: {ref} does not exist"
            assert module.endswith("_gpu"), f"{name}: {ref} is not a GPU test"


def test_the_headers_are_these_and_no_name_is_declared_twice():
    on_disk = sorted(p.name for p in A.INCLUDE.glob("*.h"))
    assert on_disk == sorted(s.header for s in _native.ABI_SURFACES) == sorted(SURFACES) and len(on_disk) == 12
    declared = [name for header in on_disk for _, name, _ in A.prototypes(header)]
    assert len(declared) == len(set(declared)) == N_EXPORTS, sorted(n for n in set(declared) if declared.count(n) > 1)
    assert sum(len(s.signatures) for s in _native.ABI_SURFACES) == N_EXPORTS           # nothing dropped by the flat union
    assert set(_native.SIGNATURES) == set(declared) and len(_native.SIGNATURES) == N_EXPORTS
    assert len(_native.ABI_SURFACES[0].signatures) == len(SURFACES["audiocut_hip.h"][2]) == N_MAIN_EXPORTS
    assert _native.ABI_SURFACES[0].header == "audiocut_hip.h"


def test_makefile_builds_every_source_and_every_object_depends_on_every_header():
    mk = (A.CSRC / "Makefile").read_text()
    (srcs,) = re.findall(r"^SRCS\s*:=(.*)$", mk, flags=re.M)
    assert sorted(srcs.split()) == sorted(p.name for p in A.CSRC.glob("*.hip"))
    (rule,) = re.findall(r"^\$\(BUILD\)/%\.o:(.*)$", mk, flags=re.M)
    deps = rule.split()
    assert "%.hip" in deps
    for folder, prefix in ((A.CSRC, ""), (A.INCLUDE, "../../include/")):
        headers = sorted(p.name for p in folder.glob("*.h"))
        assert headers
        for name in headers:
            assert prefix + name in deps or f"$(wildcard {prefix}*.h)" in rule, f"the object rule does not depend on {prefix}{name}"
