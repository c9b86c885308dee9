"""The smart-cut intent / AutoProfile layer on the host, against the reference's recorded results (tests/golden/auto_profile.json,
written by tests/golden/make_auto_profile_golden.py): every value, warning category and exception class compared with `==` on the
JSON round trip; the explicit-key bookkeeping of the runtime configuration; and the routing of `separate_and_segment`."""
import json
import types
import warnings
import wave

import numpy as np
import pytest

from audio_cut_amd import _native, api
from audio_cut_amd import config as cfg
from audio_cut_amd.config import auto_profile as AP
from audio_cut_amd.core.seamless_splitter import SeamlessSplitter, host_vocal_coverage
from audio_cut_amd.testing import profile_cases as PC

SAME = "same_as_marked"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "auto_profile.json").read_text(encoding="utf-8"))


@pytest.fixture(autouse=True)
def _clean_runtime():
    saved = cfg.snapshot()
    cfg.reset_runtime_config()
    yield
    cfg.reset_runtime_config()
    cfg.restore(saved)


def _plain(obj):
    return json.loads(json.dumps(obj, ensure_ascii=False, default=str))


def _recorded(fn):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out = {"result": _plain(fn())}
        except Exception as exc:
            out = {"error": type(exc).__name__}
    out["warnings"] = [w.category.__name__ for w in caught]
    return out


# ---- profiles, intent, alignment, style ------------------------------------------------------------------------------------------
def test_profile_tables(golden):
    assert set(golden["profiles"]) == set(AP.PROFILE_NAMES) == {"ballad", "pop", "rap", "edm"}
    for name, want in golden["profiles"].items():
        got = AP.apply_profile_overrides(name)
        assert len(got) == 25 and _plain(got) == want, name
    assert _plain(AP.default_schema_overrides()) == golden["default_schema"]
    with pytest.raises(KeyError):
        AP.apply_profile_overrides("polka")


def test_intent_grid(golden):
    rows = golden["intent"]
    assert len(rows) > 120
    for row in rows:
        sc, marks = PC.decode_value(row["smart_cut"]), set(row["explicit_keys"])
        rec = _recorded(lambda: AP.resolve_smart_cut_intent(dict(sc), explicit_keys=set(marks)))
        got = PC.pack_intent(rec["result"]) if "result" in rec else {"error": rec["error"]}
        assert (got, rec["warnings"]) == (row["intent"], row["warnings"]), row
        apply = _recorded(lambda: AP.should_apply_duration_overrides(dict(sc), explicit_keys=set(marks)))
        assert apply.get("result", apply.get("error")) == row["apply_durations"], row
    assert any(r["intent"] == {"error": "ValueError"} for r in rows)
    assert any(r["warnings"] == ["DeprecationWarning", "DeprecationWarning"] for r in rows)


def test_alignment_overrides(golden):
    block = golden["alignment"]
    for case in block["cases"]:
        if case["poles"] is None:
            weights = AP.build_style_weight_overrides(case["profile"])
            got = AP.derive_alignment_overrides(case["alignment"], weights)
        else:
            got = AP.derive_alignment_overrides(case["alignment"], case["weights"], alignment_poles=case["poles"])
        assert PC.pack_alignment(got) == case["overrides"], case
        assert (got == {}) == (case["alignment"] == 0.5)
    for key, want in block["style_weights"].items():
        name, cut_style = key.split("/")
        assert _plain(AP.build_style_weight_overrides(name, cut_style=cut_style)) == want, key
    # the poles of the configuration are the module's own
    poles = cfg.get_config("phrase_boundary.alignment_poles")
    assert poles == {"lyric": AP.LYRIC_POLE, "beat": AP.BEAT_POLE}
    w = AP.build_style_weight_overrides("rap")
    assert AP.derive_alignment_overrides(0.8, w, alignment_poles=poles) == AP.derive_alignment_overrides(0.8, w)


def test_style_estimates_and_auto_profile_overrides(golden):
    cases = {c["name"]: c for c in golden["style"]["cases"]}
    applied = golden["runtime"]["auto_applied_overrides"]
    assert set(cases) == {s["name"] for s in PC.STYLE_CASES}
    assert golden["style"]["min_margin"] >= 1e-3
    for spec in PC.STYLE_CASES:
        want = cases[spec["name"]]
        est = AP.estimate_style(PC.style_cache(spec))
        assert isinstance(est, AP.StyleEstimate)
        got = {"profile": est.profile, "confidence": est.confidence, "features": dict(est.features), "fallback_reason": est.fallback_reason}
        assert _plain(got) == want["estimate"], spec["name"]
        for key in (k for k in want if k.startswith("overrides_")):
            ov = AP.build_auto_profile_overrides(est, cut_style=key[len("overrides_"):])
            expect = dict(want[key], **{"meta.auto_profile": PC.unfold_applied(want[key]["meta.auto_profile"], applied)})
            assert applied == sorted(k for k in expect if not k.startswith("meta."))
            assert _plain(ov) == expect, (spec["name"], key)
    # a numpy beat array works like the list the cases carry
    spec = next(s for s in PC.STYLE_CASES if s["name"] == "tempo_from_beat_times")
    cache = PC.style_cache(spec)
    cache.beat_times = np.asarray(cache.beat_times, dtype=np.float32)
    assert AP.estimate_style(cache).features == cases[spec["name"]]["estimate"]["features"]


# ---- runtime configuration: explicit keys ------------------------------------------------------------------------------------------
def test_runtime_override_keys_follow_the_overrides():
    assert cfg.get_runtime_override_keys() == set()
    cfg.set_runtime_config({"smart_cut.segments": "medium", "vpbd.enabled": True})
    assert cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled"}
    keys = cfg.get_runtime_override_keys()
    keys.add("x")                                                           # a copy
    assert "x" not in cfg.get_runtime_override_keys()
    cfg.set_runtime_config({"smart_cut.alignment": "beat", "vpbd.enabled": False}, explicit=False)
    assert cfg.get_config("smart_cut.alignment") == "beat" and cfg.get_config("vpbd.enabled") is False
    assert cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled"}    # an unmarked write neither marks nor unmarks
    saved = cfg.snapshot()
    assert saved == {"smart_cut.segments": "medium", "vpbd.enabled": False, "smart_cut.alignment": "beat"} and isinstance(saved, dict)
    cfg.set_runtime_config({"smart_cut.profile": "rap", "smart_cut.alignment": 0.1})
    assert cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled", "smart_cut.profile", "smart_cut.alignment"}
    cfg.restore(saved)
    assert cfg.snapshot() == saved and cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled"}
    cfg.set_runtime_config({"smart_cut.alignment": 0.1})
    cfg.restore(dict(saved))                                                # a plain dict keeps the marks of the keys it holds
    assert cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled", "smart_cut.alignment"}
    cfg.restore(saved)
    assert cfg.get_runtime_override_keys() == {"smart_cut.segments", "vpbd.enabled"}
    cfg.restore({})
    assert cfg.get_runtime_override_keys() == set() and cfg.snapshot() == {}
    cfg.set_runtime_config({"smart_cut.segments": "few"})
    cfg.reset_runtime_config()
    assert cfg.get_runtime_override_keys() == set() and cfg.get_config("smart_cut.segments") == "medium"


def test_smart_cut_defaults_are_the_references(golden):
    row = next(r for r in golden["intent"] if set(r["smart_cut"]) == set(cfg.DEFAULTS["smart_cut"]) and r["smart_cut"]["profile"] == "auto")
    assert PC.decode_value(row["smart_cut"]) == cfg.DEFAULTS["smart_cut"] == cfg.get_config("smart_cut")
    assert PC.pack_intent(AP.resolve_smart_cut_intent(cfg.get_config("smart_cut"))) == row["intent"]
    assert not AP.should_apply_duration_overrides(cfg.get_config("smart_cut"))


# ---- `_apply_smart_cut_runtime` --------------------------------------------------------------------------------------------------
def _bare_splitter():
    """A splitter without its constructor (no separator, no device): the smart-cut runtime is host code."""
    sp = object.__new__(SeamlessSplitter)
    sp.sample_rate, sp._hip = 44100, None
    sp._last_auto_profile_meta = sp._last_intent_meta = None
    return sp


def _run_runtime(cache, vocal, dotted, *, marked):
    cfg.reset_runtime_config()
    cfg.set_runtime_config(dict(dotted), explicit=marked)
    written = {}
    real = cfg.set_runtime_config
    sp = _bare_splitter()
    try:
        cfg.set_runtime_config = lambda ov, **kw: (written.update(ov), real(ov, **kw))[1]
        rec = _recorded(lambda: sp._apply_smart_cut_runtime(cache, vocal_track=vocal))
    finally:
        cfg.set_runtime_config = real
    if "result" in rec:
        rec = {"meta": rec["result"], "warnings": rec["warnings"], "intent": _plain(sp._last_intent_meta),
               "config": {k: _plain(cfg.get_config(k)) for k in sorted(written) if k not in ("meta.auto_profile", "meta.intent")},
               "meta_in_config": [_plain(cfg.get_config(k)) == want for k, want in
                                  (("meta.auto_profile", rec["result"]), ("meta.intent", _plain(sp._last_intent_meta))) if k in written],
               "coverage": getattr(cache, "vocal_coverage_ratio", None)}
        assert sp._last_auto_profile_meta == (None if rec["meta"] is None else sp._last_auto_profile_meta)
        assert cfg.get_runtime_override_keys() >= set(written)             # the profile's own writes are marked, as the reference's are
    cfg.reset_runtime_config()
    return rec


def _both(want, make, keys):
    for marked in (True, False):
        expect = PC.expected_run(want, marked, keys)
        cache, vocal, dotted = make()
        got = _run_runtime(cache, vocal, dotted, marked=marked)
        assert got == expect, (marked, {k: (got.get(k), expect.get(k)) for k in expect if got.get(k) != expect.get(k)})
        assert got["intent"]["applied_overrides"] == expect["intent"]["applied_overrides"]


def test_runtime_cases_of_the_reference_tests(golden):
    ns = types.SimpleNamespace
    rms = lambda *v: np.asarray(v, dtype=np.float32)
    rap = lambda **kw: ns(bpm_features=ns(main_bpm=142.0), global_mdd=0.58, rms_series=rms(0.40, 0.52, 0.47), **kw)
    pop = lambda: ns(bpm_features=ns(main_bpm=108.0), global_mdd=0.38, rms_series=rms(0.2, 0.42, 0.31), vocal_coverage_ratio=0.56,
                     beat_times=rms(0.0, 0.5, 1.0))
    caches = {"auto_rhythmic_target": lambda: rap(vocal_coverage_ratio=0.82), "manual_ballad": lambda: rap(vocal_coverage_ratio=0.82),
              "coverage_from_ones": rap, "beat_many": pop, "balanced": pop}
    unit = golden["runtime"]["unit"]
    assert set(unit) == set(caches)
    for name, want in unit.items():
        vocal = None if want["vocal"] is None else (np.ones if want["vocal"] == "ones" else np.zeros)(44100, dtype=np.float32)
        _both(want, lambda: (caches[name](), vocal, PC.decode_value(want["smart_cut"])), golden["runtime"]["auto_applied_overrides"])
    assert unit["manual_ballad"]["unmarked"] != SAME                       # a default-valued target moves the planner only when set on purpose
    assert unit["coverage_from_ones"]["marked"]["coverage"] == 1.0
    assert unit["beat_many"]["marked"]["coverage"] == 0.56                  # a ratio the cache carries is kept


def test_runtime_seeded_cases(golden):
    seeded = {r["seed"]: r for r in golden["runtime"]["seeded"]}
    assert set(seeded) == {s["seed"] for s in PC.SMART_CUT_CASES} and len(seeded) >= 6
    assert golden["runtime"]["min_margin"] >= 1e-3
    differ = 0
    for spec in PC.SMART_CUT_CASES:
        want = seeded[spec["seed"]]

        def make():
            cache, _, vocal, _ = PC.smart_cut_case(spec)
            return cache, vocal, spec["smart_cut"]
        _both(want, make, golden["runtime"]["auto_applied_overrides"])
        differ += want["unmarked"] != SAME
    assert differ >= 2
    styles = {r["marked"]["meta"]["style"] for r in seeded.values() if r["marked"]["meta"]}
    assert {"pop", "edm", "rap"} <= styles and any(r["marked"]["meta"] is None for r in seeded.values())


def test_unknown_profile_warns_and_falls_back_to_pop(caplog):
    cfg.set_runtime_config({"smart_cut.profile": "shoegaze"})
    sp = _bare_splitter()
    with caplog.at_level("WARNING"):
        assert sp._apply_smart_cut_runtime(types.SimpleNamespace()) is None
    assert "shoegaze" in caplog.text and cfg.get_config("meta.profile") == "pop"
    assert cfg.get_config("quality_control.enforce_quiet_cut.search_right_ms") == 160.0


# ---- the coverage formula and `coverage_from` ------------------------------------------------------------------------------------
def test_host_coverage_formula_and_coverage_from(golden):
    cases = PC.coverage_cases(_native.PROFILE_GRID_SAMPLES)
    assert [(c["recipe"], c["n"], c["seed"]) for c in golden["coverage"]] == [tuple(c) for c in cases]
    assert max(n for _, n, _ in cases) == 2 * 4 * 256 * 2048 + 5
    sp = _bare_splitter()
    for want in golden["coverage"]:
        x = PC.coverage_signal(want["recipe"], want["n"], want["seed"])
        assert x.dtype == np.float32 and x.shape == (want["n"],)
        assert host_vocal_coverage(x) == want["coverage"], want
        peak = np.float32(np.max(np.abs(x)))
        assert int(peak.view(np.uint32)) == want["peak_bits"]
        assert _native.coverage_from(float(peak), want["count"], want["n"]) == want["coverage"]
        cache = types.SimpleNamespace()
        sp._attach_vocal_coverage(cache, x)                                  # no resident stem: the host formula
        assert cache.vocal_coverage_ratio == want["coverage"]
    assert _native.coverage_from(0.5, 0, 0) == 0.0 and _native.coverage_from(1e-9, 5, 10) == 0.0
    assert _native.coverage_from(0.5, 3, 4) == 0.75 and _native.coverage_from(0.5, 9, 4) == 1.0
    # nothing to do: no cache, a ratio already there, no stem, an empty stem
    sp._attach_vocal_coverage(None, np.ones(4, dtype=np.float32))
    kept = types.SimpleNamespace(vocal_coverage_ratio=0.25)
    sp._attach_vocal_coverage(kept, np.ones(4, dtype=np.float32))
    assert kept.vocal_coverage_ratio == 0.25
    for stem in (None, np.zeros(0, dtype=np.float32)):
        bare = types.SimpleNamespace()
        sp._attach_vocal_coverage(bare, stem)
        assert not hasattr(bare, "vocal_coverage_ratio")


def test_coverage_attribute_on_the_dataclass_cache():
    import dataclasses
    from audio_cut_amd.analysis.features_cache import TrackFeatureCache
    z = np.zeros(4, dtype=np.float32)
    cache = TrackFeatureCache(sr=44100, hop_length=441, hop_s=0.01, duration_s=0.04, rms_series=z, spectral_flatness=z, onset_envelope=z,
                              onset_strength=z, onset_frames=np.zeros(0, dtype=np.int64), rms_max=0.0, onset_max=0.0, bpm_features=None,
                              tempo_curve=None, beat_times=np.zeros(0, dtype=np.float32), global_mdd=0.0, mdd_series=z)
    _bare_splitter()._attach_vocal_coverage(cache, np.asarray([0.5, 0.0, -0.5, 0.001], dtype=np.float32))
    assert cache.vocal_coverage_ratio == 0.5
    copy = dataclasses.replace(cache, rms_max=1.0)                          # the copies the layout hook makes still work
    assert copy.rms_max == 1.0 and not hasattr(copy, "vocal_coverage_ratio")


# ---- `split_track` activation (no device needed for what is refused up front) ----------------------------------------------------
def test_smart_cut_activation_rule():
    active = SeamlessSplitter._smart_cut_active
    for mode in ("vpbd_acoustic", "vpbd_asr"):
        assert active(mode, None) is False and active(mode, True) is True and active(mode, False) is False
    cfg.set_runtime_config({"smart_cut.segments": "many"}, explicit=False)
    assert active("vpbd_asr", None) is True and active("vpbd_acoustic", False) is False
    assert active("v2.2_mdd", None) is False and active("hybrid_mdd", False) is False
    with pytest.raises(ValueError):
        active("v2.2_mdd", True)
    cfg.reset_runtime_config()
    cfg.set_runtime_config({"smart_cut": {"alignment": "beat"}})
    assert active("vpbd_acoustic", None) is True


# ---- `separate_and_segment` routing ------------------------------------------------------------------------------------------------
def _wav(path, seconds=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(44100); w.writeframes(bytes(2 * 44100 * seconds))
    return path


def _fake_result(mode, **extra):
    out = {"success": True, "mode": mode, "method": f"pure_vocal_split_{mode}", "export_plan": [], "cut_points_sec": [0.0, 2.0],
           "cut_points_samples": [0, 88200], "segment_labels": ["human"], "segment_durations": [2.0], "segment_vocal_flags": [True]}
    out.update(extra)
    return out


def test_api_intent_routing(golden, tmp_path, monkeypatch):
    src = _wav(tmp_path / "song.wav")
    seen = []

    def fake(in_path, out_dir, mode, export_types, sr, device, channels=1):
        seen.append({"mode": mode, "explicit": cfg.get_runtime_override_keys(),
                     "config": {k: cfg.get_config(k) for k in ("lyrics_alignment.enabled", "lyrics_alignment.provider", "lyrics_alignment.strict",
                                                               "smart_cut.segments", "smart_cut.alignment", "segment_layout.soft_min_s")}})
        return _fake_result(mode)

    monkeypatch.setattr(api, "_split_and_export", fake)
    cfg.set_runtime_config({"vpbd.breath_score_scale": 0.5})               # the caller's own configuration, marked
    before, marks = cfg.snapshot(), cfg.get_runtime_override_keys()
    for row in golden["api"]:
        segments = PC.decode_value(row["segments"])
        man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), segments=segments, alignment=row["alignment"],
                                       mode=row["mode"])
        call = seen[-1]
        assert call["mode"] == row["called_mode"] == man["version"] == row["version"], row
        assert _plain(man.get("intent")) == row["intent"], row
        has_intent = segments is not None or row["alignment"] is not None
        assert ("intent" in man) == has_intent
        want_cfg = {"lyrics_alignment.enabled": has_intent, "lyrics_alignment.provider": "auto" if has_intent else "disabled",
                    "lyrics_alignment.strict": False, "smart_cut.segments": segments if segments is not None else "medium",
                    "smart_cut.alignment": row["alignment"] if row["alignment"] is not None else "balanced", "segment_layout.soft_min_s": 5.0}
        assert call["config"] == want_cfg, row
        assert call["explicit"] == marks                                       # the API's own writes are not explicit
        assert cfg.snapshot() == before and cfg.get_runtime_override_keys() == marks
    assert [r["called_mode"] for r in golden["api"][:3]] == ["vpbd_asr", "vpbd_asr", "v2.2_mdd"]
    assert any(r["mode"] == "hybrid_mdd" and r["called_mode"] == "hybrid_mdd" and r["intent"] for r in golden["api"])     # an explicit mode wins

    # runtime_overrides go on top of the intent overrides, unmarked too, and a manifest is still a manifest
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), segments="few", alignment="beat",
                                   runtime_overrides={"smart_cut.segments": "many", "lyrics_alignment.provider": "fake"},
                                   layout={"soft_min_s": 6.0})
    assert seen[-1]["config"]["smart_cut.segments"] == "many" and seen[-1]["config"]["lyrics_alignment.provider"] == "fake"
    assert seen[-1]["config"]["segment_layout.soft_min_s"] == 6.0 and seen[-1]["explicit"] == marks
    assert man["intent"]["segments"] == "many" and man["intent"]["alignment"] == 1.0 and "qa_report" in man
    assert cfg.snapshot() == before and cfg.get_runtime_override_keys() == marks


def test_api_keeps_the_splitters_intent_and_restores_on_error(tmp_path, monkeypatch):
    src = _wav(tmp_path / "song.wav")
    own = {"target_duration_s": [3.0, 8.0], "segments": "many", "alignment": 1.0, "alignment_raw": "beat", "lyrics": "auto", "profile": "auto",
           "applied_overrides": ["phrase_boundary.weights.beat_affinity", "vpbd.beat_candidates.base_score"]}
    auto = {"style": "pop", "confidence": 0.7}
    monkeypatch.setattr(api, "_split_and_export", lambda i, o, mode, *a, **k: _fake_result(mode, intent=dict(own), auto_profile=dict(auto)))
    man = api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), segments="many", alignment="beat", export_manifest=True)
    assert man["intent"] == own and man["auto_profile"] == auto and man["version"] == "vpbd_asr"
    disk = json.loads((tmp_path / "out" / "SegmentManifest.json").read_text(encoding="utf-8"))
    assert disk["intent"] == own and disk["auto_profile"] == auto

    def boom(*a, **k):
        raise RuntimeError("split failed")
    monkeypatch.setattr(api, "_split_and_export", boom)
    before = cfg.snapshot()
    with pytest.raises(RuntimeError):
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), segments="few")
    assert cfg.snapshot() == before and cfg.get_runtime_override_keys() == set()
    with pytest.raises(ValueError):                                         # an invalid intent is refused before anything is split
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), alignment="loud")
    assert cfg.snapshot() == before
