"""Mode `vpbd_asr` on the host: the lyrics layer, the detector's lyrics path and the splitter's four hooks against what the
reference itself gave (tests/golden/vpbd_asr.json, written by tests/golden/make_vpbd_asr_golden.py), the provider seam, and the
16-bit conversion's known answers.  CPU only.  Everything recorded is compared exactly: it is the same float64 arithmetic in the
same order, so a difference means the restatement differs from the reference.

One representation differs on purpose and is normalised here, not tolerated: a timeline with no items and no `meta` keeps the six
keys it has always had in this library's results (`LyricsTimeline.to_dict`), where the reference's also carries `"meta": {}`."""
import json
import types

import numpy as np
import pytest

from audio_cut_amd import config as cfg
from audio_cut_amd.analysis.boundary_features import LyricsTimeline
from audio_cut_amd.core.seamless_splitter import SeamlessSplitter
from audio_cut_amd.core.vocal_phrase_boundary_detector import VocalPhraseBoundaryDetector
from audio_cut_amd.cutting.refine import CutAdjustment
from audio_cut_amd.exceptions import AudioCutError, LyricsAlignmentUnavailable, TimelineValidationError
from audio_cut_amd.lyrics import (FakeLyricsProvider, LyricsBoundaryCandidateGenerator, LyricsProvider, LyricsProviderRequest,
                                  NullLyricsProvider, attach_lyrics_to_segments, build_lyrics_provider)
from audio_cut_amd.lyrics import models as lyrics_models
from audio_cut_amd.testing.lyrics_cases import CASE_SECONDS, asr_case
from audio_cut_amd.testing.vpbd_inputs import FixedPauses, vpbd_case
from audio_cut_amd.utils.audio_export import pcm_bytes_host

SR = 44100
FIXTURE_KEY = "lyrics_alignment.fixture_path"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "vpbd_asr.json").read_text(encoding="utf-8"))


def _plain(obj):
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


def _norm_timeline(d):
    """the reference's payload of an EMPTY timeline, as this library writes it (module docstring)."""
    d = dict(d)
    if not (d.get("words") or d.get("sentences") or d.get("vad_regions") or d.get("meta")):
        d.pop("meta", None)
    return d


def _norm_result(rec):
    rec = json.loads(json.dumps(rec))
    rec["lyrics_alignment"]["timeline"] = _norm_timeline(rec["lyrics_alignment"]["timeline"])
    return rec


def _detect(overrides, payload, tmp_path, *, cache, pauses, vocal, sr=SR, input_path="track.wav", detector=None, mode="vpbd_asr"):
    ov = dict(overrides)
    if payload is not None:
        path = tmp_path / "timeline.json"
        path.write_text(json.dumps(payload, ensure_ascii=False), encoding="utf-8")
        ov[FIXTURE_KEY] = str(path)
    saved = cfg.snapshot()
    cfg.set_runtime_config(ov)
    try:
        det = detector or VocalPhraseBoundaryDetector(sr)
        res = det.detect(mode=mode, vocal_track=vocal, original_audio=vocal, pure_vocal_detector=FixedPauses(pauses),
                         feature_cache=cache, vad_segments=None, input_path=input_path, output_dir="")
    finally:
        cfg.restore(saved)
    return res


# ---- (a) detect with the fake provider ----------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(6))
def test_detect_matches_the_reference(golden, tmp_path, index):
    case = golden["detect"][index]
    cache, pauses, vocal, payload = asr_case(case["seed"], breaths=case["breaths"])
    res = _detect(case["overrides"], payload, tmp_path, cache=cache, pauses=pauses, vocal=vocal)
    want = _norm_result(case["result"])
    got = _plain({"boundary_detection": res.boundary_detection, "lyrics_alignment": res.lyrics_alignment})
    for block in ("lyrics_alignment", "boundary_detection"):
        for key in want[block]:
            assert got[block][key] == want[block][key], (block, key)
        assert got[block].keys() == want[block].keys()
    assert res.lyrics_alignment["word_count"] > 0 and res.boundary_detection["candidate_counts"]["lyrics"] > 0
    assert [c.to_dict() for c in res.selected_candidates] == res.boundary_detection["selected"]


def test_detect_fallbacks_match_the_reference(golden, tmp_path):
    for case in golden["fallbacks"]:
        cache, pauses, vocal, good = asr_case(case["seed"])
        want = dict(case["result"])
        if "error" in want:
            with pytest.raises(AudioCutError) as err:
                _detect(case["overrides"], case["timeline"], tmp_path, cache=cache, pauses=pauses, vocal=vocal)
            assert type(err.value).__name__ == want["error"] and str(err.value) == want["message"], case["name"]
            continue
        res = _detect(case["overrides"], case["timeline"], tmp_path, cache=cache, pauses=pauses, vocal=vocal)
        got = _plain({"boundary_detection": res.boundary_detection, "lyrics_alignment": res.lyrics_alignment})
        # its candidates are those of the run it falls back to (the generator asserts the same of the reference)
        if want.pop("candidates_as") == "acoustic":
            twin = _detect({"vpbd.candidate_debug_json": False}, None, tmp_path, cache=cache, pauses=pauses, vocal=vocal, mode="vpbd_acoustic")
        else:
            twin = _detect(dict(case["overrides"]), good, tmp_path, cache=cache, pauses=pauses, vocal=vocal)
        for key in ("selected", "suppressed"):
            assert got["boundary_detection"].pop(key) == _plain(twin.boundary_detection[key]), (case["name"], key)
        assert got == _norm_result(want), case["name"]


# ---- (b) the timeline model ------------------------------------------------------------------------------------------------
def test_timeline_from_dict_matches_the_reference(golden):
    for case in golden["from_dict"]:
        want = case["result"]
        tag = (case["name"], case["strict"])
        if "error" in want:
            with pytest.raises(TimelineValidationError) as err:
                LyricsTimeline.from_dict(json.loads(json.dumps(case["payload"])), strict=case["strict"])
            assert type(err.value).__name__ == want["error"] and str(err.value) == want["message"], tag
        else:
            got = LyricsTimeline.from_dict(json.loads(json.dumps(case["payload"])), strict=case["strict"])
            assert _plain(got.to_dict()) == _norm_timeline(want["timeline"]), tag
            again = LyricsTimeline.from_dict(got.to_dict(), strict=True)          # a payload survives its own round trip
            assert again.to_dict() == got.to_dict(), tag


def test_empty_timeline_keeps_its_payload_and_its_import_path():
    assert LyricsTimeline is lyrics_models.LyricsTimeline
    assert LyricsTimeline(duration_s=3.0, source="none").to_dict() == {
        "duration_s": 3.0, "source": "none", "words": [], "sentences": [], "vad_regions": [], "warnings": []}
    with pytest.raises(TimelineValidationError):
        lyrics_models.Word("", 0.0, 1.0)
    with pytest.raises(TimelineValidationError):
        LyricsTimeline(duration_s=2.0, words=[lyrics_models.Word("a", 1.0, 3.0)])


# ---- (c), (d) the splitter's hooks -----------------------------------------------------------------------------------------
def _host_splitter(sr=SR):
    stub = types.SimpleNamespace(_primary_backend=None)
    return SeamlessSplitter(sr, separator=stub)


def test_restore_guard_points_matches_the_reference(golden):
    splitter = _host_splitter()
    restores = 0
    for case in golden["restore"]:
        adjs = [CutAdjustment(*a) for a in case["adjustments"]]
        points, got = splitter._restore_guard_points_outside_lyrics_words(
            list(case["points"]), adjs, [tuple(x) for x in case["word_intervals"]], sample_count=case["sample_count"], min_gap_s=case["min_gap_s"])
        rec = {"points": [int(p) for p in points],
               "adjustments": None if got is None else [[a.raw_time, a.guard_time, a.final_time, a.score, a.guard_shift_ms, a.final_shift_ms] for a in got]}
        assert _plain(rec) == case["result"], case["name"]
        restores += got is not None
    assert restores >= 2


def test_collect_lyrics_intervals_and_boundaries_match_the_reference(golden):
    for case in golden["collect"]:
        assert _plain(SeamlessSplitter._collect_lyrics_word_intervals(case["input"])) == case["word_intervals"]
        assert _plain(SeamlessSplitter._collect_lyrics_boundary_times(case["input"])) == case["boundary_times"]
    # the reference's own known answer (tests/integration/test_pipeline_vpbd_asr_fake_provider.py:244-262): word edges are no priors
    assert SeamlessSplitter._collect_lyrics_boundary_times({"timeline": {
        "words": [{"text": "a", "start_s": 1.0, "end_s": 1.4}, {"text": "b", "start_s": 2.0, "end_s": 2.4}],
        "sentences": [{"text": "a b", "start_s": 1.0, "end_s": 2.4}], "vad_regions": [{"start_s": 0.9, "end_s": 2.5, "kind": "singing"}]}}) == [0.9, 2.4, 2.5]


# ---- (e) attachment and manifest segments ------------------------------------------------------------------------------------
def test_attach_and_manifest_segments_match_the_reference(golden, tmp_path):
    from audio_cut_amd.api import _build_manifest
    rec = golden["attach"]
    timeline = LyricsTimeline.from_dict(rec["timeline"], strict=True)
    assert _plain(attach_lyrics_to_segments(rec["segments"], timeline)) == rec["attached"]
    assert "lyrics" not in rec["segments"][0]                                       # the input rows are copied, not touched
    src = tmp_path / "song.wav"
    src.write_bytes(b"RIFF")
    result = dict(rec["manifest_result"], lyrics_alignment=dict(rec["manifest_result"]["lyrics_alignment"], timeline=timeline.to_dict()))
    man = _build_manifest(result=result, input_path=src, export_dir=tmp_path / "out", mode="vpbd_asr", sample_rate=SR,
                          channels=1, layout_cfg={})
    assert _plain(man["segments"]) == rec["manifest_segments"]
    # a result whose alignment did not run keeps its rows as they were
    off = dict(result, lyrics_alignment=dict(result["lyrics_alignment"], enabled=False))
    man = _build_manifest(result=off, input_path=src, export_dir=tmp_path / "out", mode="vpbd_asr", sample_rate=SR, channels=1, layout_cfg={})
    assert all("lyrics" not in s for s in man["segments"])


# ---- (f) the reference's integration scenarios, detector half (the whole mode runs in the GPU suite) -------------------------
def test_integration_priority_scenario_matches_the_reference(golden, tmp_path):
    case = golden["integration"]["priority"]
    cache = types.SimpleNamespace(beat_times=np.arange(0.0, 8.001, 0.5, dtype=np.float32), rms_series=np.full(160, 0.8, dtype=np.float32),
                                  hop_s=0.05, duration_s=8.0, mdd_series=np.full(160, 0.5, dtype=np.float32))
    res = _detect(case["config"], case["timeline"], tmp_path, cache=cache, pauses=[types.SimpleNamespace(**p) for p in case["pauses"]],
                  vocal=np.zeros(int(case["sample_rate"] * case["seconds"]), dtype=np.float32), sr=case["sample_rate"], input_path="sample.wav")
    got = _plain({"boundary_detection": res.boundary_detection, "lyrics_alignment": res.lyrics_alignment})
    assert got == _norm_result(case["result"])


# ---- nothing else changes ------------------------------------------------------------------------------------------------------
def test_acoustic_results_are_the_parents(golden_dir, tmp_path):
    g = np.load(golden_dir / "vpbd.npz")
    for case, seed in enumerate((31, 32, 33)):
        cache, pauses, vocal = vpbd_case(seed)
        outs = []
        for mode in ("vpbd_acoustic", "vpbd_asr"):          # lyrics alignment is off by default: `vpbd_asr` resolves to the acoustic pool
            res = VocalPhraseBoundaryDetector(SR).detect(mode=mode, vocal_track=vocal, original_audio=vocal, pure_vocal_detector=FixedPauses(pauses),
                                                         feature_cache=cache, vad_segments=None, input_path="x.wav", output_dir=str(tmp_path))
            assert np.array_equal(np.array([[c.t, c.score] for c in res.selected_candidates]), g[f"c{case}_selected"])
            assert np.array_equal(np.array([[c.t, c.score] for c in res.planner_result.suppressed_candidates]).reshape(-1, 2), g[f"c{case}_suppressed"])
            assert np.array_equal(np.array([[c.features[k] for k in sorted(c.features)] for c in res.selected_candidates]), g[f"c{case}_features"])
            counts = res.boundary_detection["candidate_counts"]
            assert [counts[k] for k in ("acoustic", "beat", "merged", "total", "selected", "suppressed")] == g[f"c{case}_counts"].tolist()
            assert counts["lyrics"] == counts["lyrics_pooled"] == counts["lyrics_soft_prior"] == 0
            assert res.lyrics_alignment["timeline"] == {"duration_s": 60.0, "source": "none", "words": [], "sentences": [], "vad_regions": [],
                                                        "warnings": []}
            assert not list(tmp_path.glob("*_vocal_for_asr.wav"))
            # the directory `split_track` forwards places the ASR copy alone: no debug JSON, `candidate_debug_path` None as before
            quiet = VocalPhraseBoundaryDetector(SR).detect(mode=mode, vocal_track=vocal, original_audio=vocal, pure_vocal_detector=FixedPauses(pauses),
                                                           feature_cache=cache, vad_segments=None, input_path="x.wav",
                                                           asr_output_dir=str(tmp_path / f"export_{mode}_{seed}"))
            assert quiet.boundary_detection["candidate_debug_path"] is None and not (tmp_path / f"export_{mode}_{seed}").exists()
            assert quiet.boundary_detection["selected"] == res.boundary_detection["selected"]
            outs.append(res)
        assert outs[1].boundary_detection["actual_mode"] == "vpbd_acoustic" and outs[1].lyrics_alignment["fallback_reason"] == "lyrics_alignment_disabled"
        assert outs[1].lyrics_alignment["enabled"] is False and outs[1].lyrics_alignment["provider"] == "disabled"
        assert outs[0].boundary_detection["selected"] == outs[1].boundary_detection["selected"]


# ---- the provider seam -----------------------------------------------------------------------------------------------------------
def test_provider_selection_table(tmp_path):
    for name in ("disabled", "none", "null", "", " Disabled "):
        p = build_lyrics_provider({"provider": name})
        assert isinstance(p, NullLyricsProvider) and p.reason == "lyrics alignment disabled"
    assert build_lyrics_provider({}).reason == "lyrics alignment disabled"
    p = build_lyrics_provider({"provider": "fake"})
    assert isinstance(p, NullLyricsProvider) and p.reason == "fake lyrics provider requires fixture_path"
    p = build_lyrics_provider({"provider": "FAKE", "fixture_path": str(tmp_path / "t.json")})
    assert isinstance(p, FakeLyricsProvider) and p.name == "fake" and p.fixture_path == tmp_path / "t.json"
    for name in ("sidecar", "cli", "auto"):
        p = build_lyrics_provider({"provider": name, "fire_red": {"endpoint": "http://127.0.0.1:1", "cli": {"executable": "firered"}}})
        assert isinstance(p, NullLyricsProvider) and "not built" in p.reason and name in p.reason
        with pytest.raises(LyricsAlignmentUnavailable):
            p.align(LyricsProviderRequest(vocal_path=None, duration_s=1.0, strict=True))
        empty = p.align(LyricsProviderRequest(vocal_path=None, duration_s=1.0, strict=False))
        assert empty.source == "null" and empty.warnings == [p.reason] and not empty.words
    assert build_lyrics_provider({"provider": "whisper"}).reason == "unsupported lyrics provider: whisper"
    assert "fixture_path" not in cfg.get_config("lyrics_alignment", {})               # the defaults gained no key


class _Recorder(LyricsProvider):
    name = "host_app"

    def __init__(self, payload=None, error=None):
        self.payload, self.error, self.requests = payload, error, []

    def align(self, request):
        self.requests.append(request)
        if self.error is not None:
            raise self.error
        return LyricsTimeline.from_dict(dict(self.payload), strict=request.strict)


def test_injected_provider_is_used_and_failures_fall_back(tmp_path):
    cache, pauses, vocal, payload = asr_case(31)
    on = {"lyrics_alignment.enabled": True, "lyrics_alignment.provider": "cli"}          # what the configuration names is not consulted
    det = VocalPhraseBoundaryDetector(SR)
    det.lyrics_provider = _Recorder(payload)
    res = _detect(on, None, tmp_path, cache=cache, pauses=pauses, vocal=vocal, detector=det)
    (req,) = det.lyrics_provider.requests
    assert req.sample_rate == 16000 and req.duration_s == CASE_SECONDS and req.strict is False
    assert req.vocal_path is None and "pcm16" not in req.meta                          # host-only: no device state, no copy
    assert res.lyrics_alignment["provider"] == "host_app" and res.boundary_detection["actual_mode"] == "vpbd_asr"
    want = LyricsBoundaryCandidateGenerator().generate(LyricsTimeline.from_dict(payload, strict=True))
    assert res.boundary_detection["candidate_counts"]["lyrics"] == len(want) > 0
    assert res.lyrics_alignment["word_count"] == len(payload["words"])

    for error, reason in ((LyricsAlignmentUnavailable("engine offline"), "lyrics_alignment_unavailable"), (RuntimeError("boom"), "boom")):
        det.lyrics_provider = _Recorder(error=error)
        res = _detect(on, None, tmp_path, cache=cache, pauses=pauses, vocal=vocal, detector=det)
        assert res.boundary_detection["actual_mode"] == "vpbd_acoustic" and res.lyrics_alignment["fallback_reason"] == reason
        assert res.lyrics_alignment["provider"] == "host_app" and res.boundary_detection["candidate_counts"]["lyrics"] == 0
        acoustic = VocalPhraseBoundaryDetector(SR).detect(mode="vpbd_acoustic", vocal_track=vocal, original_audio=vocal,
                                                          pure_vocal_detector=FixedPauses(pauses), feature_cache=cache, vad_segments=None)
        assert res.boundary_detection["selected"] == acoustic.boundary_detection["selected"]
        with pytest.raises(type(error)):
            _detect(dict(on, **{"lyrics_alignment.strict": True}), None, tmp_path, cache=cache, pauses=pauses, vocal=vocal, detector=det)
        assert det.lyrics_provider.requests[-1].strict is True


# ---- the 16-bit conversion (libsndfile's clipping float -> PCM_16, `pcm_bytes_host`) -------------------------------------------
def _pcm16(values):
    data, width = pcm_bytes_host(np.asarray(values, dtype=np.float32), "PCM_16")
    assert width == 2
    return data.view("<i2").astype(np.int64)


def test_pcm16_known_answers():
    step = 2.0 ** -15
    assert _pcm16([0.0, -0.0]).tolist() == [0, 0]
    assert _pcm16([1.0, -1.0]).tolist() == [32767, -32768]
    assert _pcm16([1.0 - step, -(1.0 - step)]).tolist() == [32767, -32767]
    assert _pcm16([1.3, -1.3, np.inf, -np.inf]).tolist() == [32767, -32768, 32767, -32768]
    assert _pcm16([np.nan]).tolist() == [0]
    # a floor of x * 2^15, not a rounding: the word is the top two bytes of lrintf(x * 2^31)
    k = 1234
    below, above = np.nextafter(np.float32(k * step), np.float32(-1)), np.nextafter(np.float32(k * step), np.float32(1))
    assert _pcm16([k * step, below, above, (k + 0.999) * step]).tolist() == [k, k - 1, k, k]
    assert _pcm16([-k * step, np.nextafter(np.float32(-k * step), np.float32(-1)), np.nextafter(np.float32(-k * step), np.float32(1))]).tolist() == [-k, -k - 1, -k]
    assert _pcm16([0.5 * step, -0.5 * step, 2.0 ** -33, -(2.0 ** -33)]).tolist() == [0, -1, 0, 0]
    sweep = np.sort(np.linspace(-1.4, 1.4, 200001).astype(np.float32))
    out = _pcm16(sweep)
    assert np.all(np.diff(out) >= 0) and out[0] == -32768 and out[-1] == 32767
