"""True-stereo separation end to end (GPU box only): `infer_chunk` on a (2, n) chunk against the CPU oracle, mono-equivalence of
`separate_track` on L == R, `split_track` on a stereo song against an oracle run built here, and `audio.channels: 2` through
`separate_and_segment`."""
import json
import wave

import numpy as np
import pytest
import torch

from audio_cut_amd import config as CFG
from audio_cut_amd.testing import signals
from oracle import chunking as OC, detector as OD, e2e as OE, features as OF, refine as OR, separator as OS, vad as OV
from oracle.config import get_config as oracle_config

pytestmark = pytest.mark.gpu
SR = 44100
STEM_RTOL = 1e-4


@pytest.fixture(scope="module")
def weights():
    from audio_cut_amd.separation.tfc_tdf import TfcTdfSpec, synth_weights
    return synth_weights(TfcTdfSpec(), seed=0)


def _backend(hip, weights, output_type="vocal", **kw):
    from audio_cut_amd.separation.backends import MDX23HipBackend
    saved = CFG.snapshot()
    try:
        CFG.set_runtime_config({"enhanced_separation.mdx23.output_type": output_type})
        b = MDX23HipBackend(weights=weights, ctx=hip, **kw)
    finally:
        CFG.restore(saved)
    b.load_model()
    assert b.get_output_type() == output_type
    return b


def test_infer_chunk_true_stereo_against_oracle(hip_ctx, weights):
    chunk = signals.c2_song(10.0, seed=6, stereo=True)
    assert not np.array_equal(chunk[0], chunk[1])
    batch, st, orig = OC.mdx_windows(chunk)
    wave = OS.mdx_istft(OS.unet_forward(OS.mdx_stft(batch), weights))
    for output_type in ("vocal", "instrumental"):
        ref_v, ref_i = OC.mdx_assemble(wave, st, orig, output_type)
        out = _backend(hip_ctx, weights, output_type).infer_chunk(chunk)
        assert out.vocal.shape == out.instrumental.shape == (chunk.shape[1],)
        err_v = float(np.max(np.abs(out.vocal - ref_v)) / np.max(np.abs(ref_v)))
        err_i = float(np.max(np.abs(out.instrumental - ref_i)) / np.max(np.abs(ref_i)))
        print(f"infer_chunk stereo {output_type}: vocal {err_v:.3e}, instrumental {err_i:.3e}")
        assert err_v < STEM_RTOL and err_i < STEM_RTOL


@pytest.mark.parametrize("items_per_forward", [64, 7])
def test_separate_track_on_identical_channels_is_the_mono_path(hip_ctx, weights, items_per_forward):
    from audio_cut_amd.utils.gpu_pipeline import chunk_schedule
    x = signals.c2_song(30.0, seed=12)
    plans = chunk_schedule(len(x) / SR)
    for output_type in ("vocal", "instrumental"):
        b = _backend(hip_ctx, weights, output_type, max_items_per_forward=items_per_forward)
        mono = b.separate_track(hip_ctx.to_device(x), SR, plans)
        st = b.separate_track(hip_ctx.to_device(np.stack([x, x])), SR, plans)
        assert items_per_forward == 64 or mono.n_items % items_per_forward != 0        # 7: a ragged last forward
        assert torch.equal(st.vocal, mono.vocal) and torch.equal(st.instrumental, mono.instrumental), output_type
        assert mono.vocal_stereo is None and st.vocal_stereo.shape == (2, len(x))
        # the network's L and R outputs differ even for identical inputs; the mono stems are their channel means up to rounding
        tol = float(st.vocal_stereo.abs().max()) * 1e-6
        assert torch.allclose((st.vocal_stereo[0] + st.vocal_stereo[1]) * 0.5, st.vocal, rtol=0, atol=tol)
        if output_type == "vocal":
            assert torch.equal(st.chunk_vocal, mono.chunk_vocal)
        else:
            # mono computes mix - mean(wave); stereo takes mdx_assemble's mean(mix - wave): equal up to one rounding
            assert torch.allclose(st.chunk_vocal, mono.chunk_vocal, rtol=0, atol=float(mono.chunk_vocal.abs().max()) * 1e-6)


def _oracle_stereo_run(stereo, sr, w):
    """oracle.e2e.run_track with the network fed true-stereo chunks and everything else fed the mono mix."""
    mono = (stereo[0] + stereo[1]) * np.float32(0.5)
    feat = OF.ChunkFeatureOracle(sr)
    cvad = OV.ChunkVadOracle(sr, float(oracle_config("advanced_vad.silero_merge_gap_ms", 120.0)),
                             float(oracle_config("advanced_vad.focus_window_pad_s", 0.2)), OV.energy_gate_vad(sr))
    total = stereo.shape[1]
    plans = OC.chunk_plan(total / float(sr))
    outs, kept = [], []
    for plan, (cs, ce, es, ee) in zip(plans, OC.plan_sample_ranges(plans, sr, total)):
        if ce <= cs:
            continue
        voc, inst = OS.infer_chunk(np.ascontiguousarray(stereo[:, cs:ce]), w)
        cvad.process_chunk(plan, voc, sr)
        if ee > es:
            feat.add_chunk(plan, mono[cs:ce], sr)
        outs.append((voc, inst)); kept.append((cs, ce, es, ee))
    vocal, inst = OC.overlap_add(total, kept, outs)
    vad_segments = cvad.finalize()
    cache = feat.finalize(mono)
    markers = OD.vocal_presence_markers(vocal, sr)
    pol: list = []
    pauses, _, bounds = OE.detect_and_finalize(mono, vocal, sr, cache, vad_segments, markers, {}, policy_out=pol)
    return mono, vocal, inst, vad_segments, cache, pauses, bounds, pol[0]


def test_split_track_stereo_against_oracle(hip_ctx, weights):
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    st = signals.c2_song(30.0, seed=3, stereo=True)
    sp = SeamlessSplitter(SR, separator=EnhancedVocalSeparator(SR, backend=_backend(hip_ctx, weights)))
    res = sp.split_track(st)
    OR.LEGACY_PROMOTION = True
    mono, vocal, inst, vad_segments, cache, pauses, bounds, policy = _oracle_stereo_run(st, SR, weights)
    assert np.array_equal(res["mono_mix"], mono) and np.array_equal(mono, np.mean(st, axis=0))
    assert torch.equal(res["device_state"]["mix"].cpu(), torch.from_numpy(mono))      # the device mix is the same bits
    err_v = float(np.max(np.abs(res["vocal_track"] - vocal)) / np.max(np.abs(vocal)))
    err_i = float(np.max(np.abs(res["instrumental_track"] - inst)) / np.max(np.abs(inst)))
    print(f"stereo split_track stems: vocal {err_v:.3e}, instrumental {err_i:.3e}")
    assert err_v < STEM_RTOL and err_i < STEM_RTOL
    # the stereo stems: their channel means are the mono stems up to the (w0 + w1) * 0.5 rounding, and they are on the host too
    vs, is_ = res["vocal_track_stereo"], res["instrumental_track_stereo"]
    assert vs.shape == is_.shape == (2, st.shape[1])
    assert np.array_equal(vs, res["device_state"]["vocal_stereo"].cpu().numpy())
    assert np.array_equal(is_, res["device_state"]["instrumental_stereo"].cpu().numpy())
    scale = max(float(np.max(np.abs(vs))), float(np.max(np.abs(st))))
    assert float(np.max(np.abs((vs[0] + vs[1]) * 0.5 - res["vocal_track"]))) <= 1e-6 * scale
    assert float(np.max(np.abs(vs + is_ - st))) <= 1e-6 * scale                          # stem + (mix - stem) = mix per channel
    # integers exact: VAD segments, onset frames, pauses, boundaries, cuts
    assert res["vad_segments"] == vad_segments
    assert np.array_equal(res["feature_cache"].onset_frames, cache.onset_frames)
    got_p = [(p.start_time, p.end_time, p.cut_point) for p in res["pauses"]]
    assert got_p == [(p.start_time, p.end_time, p.cut_point) for p in pauses]
    assert res["sample_boundaries"] == bounds
    assert res["cuts_samples"] == policy.cuts and res["segment_vocal_flags"] == policy.flags


def test_stereo_is_refused_by_the_track_pipeline(hip_ctx, weights):
    import threading
    from audio_cut_amd.core.enhanced_vocal_separator import EnhancedVocalSeparator
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    sp = SeamlessSplitter(SR, separator=EnhancedVocalSeparator(SR, backend=_backend(hip_ctx, weights)))
    with pytest.raises(ValueError, match="mono"):
        sp.split_track(np.zeros((2, SR), np.float32), separation_gate=threading.Lock())


def test_separate_and_segment_with_two_channels(hip_ctx, tmp_path):
    import scipy.signal
    from audio_cut_amd import api
    from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
    from audio_cut_amd.utils import audio_export as AE
    st = signals.c2_song(14.0, seed=9, stereo=True)
    st48 = np.stack([scipy.signal.resample_poly(ch, 160, 147) for ch in st]).astype(np.float32)
    src = tmp_path / "song48.wav"
    pcm = np.clip(np.rint(st48.T * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(src), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(pcm.tobytes())
    out_dir = tmp_path / "out"
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(out_dir), export_manifest=True,
                                   runtime_overrides={"audio.channels": 2})
    res = api.last_result()
    assert man["audio"]["channels"] == 2 and json.loads((out_dir / "SegmentManifest.json").read_text())["audio"]["channels"] == 2
    # the same inputs straight into split_track: the loader's stereo track, each channel resampled on the device
    loaded, file_sr = api.load_audio_stereo(str(src))
    st44 = torch.stack([hip_ctx.resample_poly(hip_ctx.to_device(loaded[c]), SR, file_sr) for c in range(2)]).cpu().numpy()
    direct = SeamlessSplitter(SR).split_track(st44)
    assert res["cut_points_samples"] == direct["cuts_samples"]
    files = res["saved_files"]
    assert files and len(res["mix_segment_files"]) == len(res["vocal_segment_files"]) == res["num_segments"]
    for f in files:
        with wave.open(f, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 3, SR), f
    cuts = direct["cuts_samples"]
    spans = [tuple(sp) for sp in direct.get("segment_spans", list(zip(cuts[:-1], cuts[1:])))]
    assert len(spans) == len(res["mix_segment_files"])
    mix_bytes, _ = AE.pcm_bytes_host(st44.T, "PCM_24")
    for f, (lo, hi) in zip(res["mix_segment_files"], spans):
        with open(f, "rb") as fh:
            assert fh.read() == AE.wav_header(hi - lo, SR, 2, 3) + mix_bytes[lo * 6: hi * 6].tobytes(), f
    voc_bytes, _ = AE.pcm_bytes_host(direct["vocal_track_stereo"].T, "PCM_24")
    with open(res["full_vocal_file"], "rb") as fh:
        assert fh.read() == AE.wav_header(st44.shape[1], SR, 2, 3) + voc_bytes.tobytes()
