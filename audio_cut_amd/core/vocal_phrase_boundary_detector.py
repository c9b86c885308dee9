"""VPBD unified candidate pool (modes `vpbd_acoustic` and `vpbd_asr`) — mirrors the reference's
`src/vocal_smart_splitter/core/vocal_phrase_boundary_detector.py:49-411`:
acoustic pauses from `PureVocalPauseDetector` (HIP kernels) + weak beat candidates in high-energy bars + the lyrics candidates of
a provider's timeline + +-120 ms fusion + feature scoring (MDD valleys, cached-RMS vocal risk, beat affinity/conflict, word gaps,
sentence ends, inside-word and singing penalties) + the global DP planner.  Host logic over <= a few hundred candidates; the
heavy lifting (stems, caches, pauses) is already in HBM-resident kernels upstream.

`vpbd_asr` with `lyrics_alignment.enabled` false (the shipped default, `unified.yaml:28-29`) resolves to `vpbd_acoustic` with
`fallback_reason="lyrics_alignment_disabled"` (`:78-80`).  Switched on, the mode asks a `LyricsProvider` (`lyrics/providers.py`)
for the track's timeline; what it hands the provider is the vocal stem as 16 kHz 16-bit PCM, made on the GPU in one kernel from
the resident stem (`ac_resample_poly_pcm16`, reference `:388-411`).  The ASR engines themselves are external: a host application
sets its own provider as `VocalPhraseBoundaryDetector.lyrics_provider`.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np

from ..analysis.boundary_features import BoundaryFeatureExtractor, LyricsTimeline
from ..exceptions import LyricsAlignmentUnavailable
from ..lyrics.candidates import LyricsBoundaryCandidateGenerator
from ..lyrics.providers import LyricsProvider, LyricsProviderRequest, build_lyrics_provider
from ..config import get_config
from ..cutting.beat_candidates import generate_beat_candidates
from ..cutting.cut_candidate import CandidateSource, CutCandidate, adapt_legacy_acoustic_candidates
from ..cutting.global_cut_planner import GlobalCutPlanner, GlobalCutPlannerConfig, GlobalCutPlanResult
from ..cutting.phrase_boundary_scorer import PhraseBoundaryScorer, write_candidate_debug_json


@dataclass
class VPBDDetectionResult:
    selected_candidates: List[CutCandidate]
    planner_result: GlobalCutPlanResult
    boundary_detection: Dict[str, Any]
    lyrics_alignment: Dict[str, Any]


def _section(name: str) -> Dict[str, Any]:
    try:
        v = get_config(name, {})
    except Exception:
        return {}
    return dict(v) if isinstance(v, dict) else {}


def _planner_config() -> GlobalCutPlannerConfig:
    c = _section("global_planner")
    return GlobalCutPlannerConfig(
        hard_min_s=float(c.get("hard_min_s", 2.0)), hard_max_s=float(c.get("hard_max_s", 18.0)),
        target_min_s=float(c.get("target_min_s", 5.0)), target_max_s=float(c.get("target_max_s", 12.0)),
        duration_penalty_weight=float(c.get("duration_penalty_weight", 0.15)),
        vocal_risk_weight=float(c.get("vocal_risk_weight", 0.25)), beat_conflict_weight=float(c.get("beat_conflict_weight", 0.15)),
        max_candidates_per_second=float(c.get("max_candidates_per_second", 2.0)), rescue_enabled=bool(c.get("rescue_enabled", True)))


class VocalPhraseBoundaryDetector:
    ASR_SAMPLE_RATE = 16000

    def __init__(self, sample_rate: int = 44100) -> None:
        self.sample_rate = sample_rate
        self.lyrics_provider: Optional[LyricsProvider] = None      # a host application's own ASR; None: `build_lyrics_provider`

    def detect(self, *, mode: str, vocal_track: np.ndarray, original_audio: np.ndarray, pure_vocal_detector: Any,
               feature_cache: Optional[Any], vad_segments: Optional[List[Dict[str, float]]], input_path: str = "",
               output_dir: str = "", device_state: Optional[Dict[str, Any]] = None,
               asr_output_dir: Optional[str] = None) -> VPBDDetectionResult:
        """`output_dir`: where the candidate debug JSON (`vpbd.candidate_debug_json`) and the ASR copy go, as in the reference.
        `asr_output_dir`, when given, is where the ASR copy goes instead: `split_track` passes the export directory through it
        alone, so that no mode starts writing the debug JSON into a user's export directory."""
        sr = self.sample_rate
        duration_s = len(original_audio) / float(sr) if sr > 0 else 0.0
        actual_mode, fallback_reason = mode, None
        timeline = LyricsTimeline(duration_s=duration_s, source="none")
        vpbd_cfg = _section("vpbd")
        pool = str(vpbd_cfg.get("candidate_pool", "unified")).strip().lower()
        if pool not in {"unified", "legacy"}:
            pool = "unified"
        unified = pool == "unified"
        lyrics_cfg = _section("lyrics_alignment")
        strict = bool(lyrics_cfg.get("strict", False))
        lyrics_enabled = bool(lyrics_cfg.get("enabled", False)) and mode == "vpbd_asr"
        provider_name = str(lyrics_cfg.get("provider", "disabled"))
        lyrics: List[CutCandidate] = []
        state = device_state or {}
        if mode == "vpbd_asr" and not lyrics_enabled:
            actual_mode, fallback_reason = "vpbd_acoustic", "lyrics_alignment_disabled"
        elif mode == "vpbd_asr":                 # reference `:83-116`
            provider = self.lyrics_provider
            if provider is None:
                provider = build_lyrics_provider(dict(lyrics_cfg, fire_red=_section("fire_red")))
            provider_name = provider.name
            try:
                if provider.name == "null":
                    raise LyricsAlignmentUnavailable(str(getattr(provider, "reason", "lyrics alignment unavailable")))
                asr_path, pcm16 = self._asr_vocal_copy(state, input_path, output_dir if asr_output_dir is None else asr_output_dir)
                timeline = provider.align(LyricsProviderRequest(
                    vocal_path=asr_path, duration_s=duration_s, sample_rate=self.ASR_SAMPLE_RATE, strict=strict,
                    meta={} if pcm16 is None else {"pcm16": pcm16}))
                lyrics = LyricsBoundaryCandidateGenerator().generate(timeline)
            except LyricsAlignmentUnavailable:
                if strict:
                    raise
                actual_mode, fallback_reason = "vpbd_acoustic", "lyrics_alignment_unavailable"
            except Exception as exc:
                if strict:
                    raise
                actual_mode, fallback_reason = "vpbd_acoustic", str(exc)

        acoustic = self._build_acoustic_candidates(vocal_track=vocal_track, original_audio=original_audio,
                                                   pure_vocal_detector=pure_vocal_detector, feature_cache=feature_cache,
                                                   vad_segments=vad_segments, enable_mdd=True, include_breath_candidates=unified,
                                                   device_state=state)
        beats = self._build_beat_candidates(vocal_track=vocal_track, feature_cache=feature_cache, duration_s=duration_s,
                                            device_state=state) if unified else []
        pooled = lyrics if unified else []        # the legacy pool keeps the timeline for scoring only
        merged = self._merge_candidate_pool(acoustic, pooled, beats)
        scored = self._score_candidates(candidates=merged, timeline=timeline, feature_cache=feature_cache)
        debug_path: Optional[str] = None
        if bool(vpbd_cfg.get("candidate_debug_json", False)) and output_dir:
            debug_path = str(Path(output_dir) / "vpbd_candidate_debug.json")
            write_candidate_debug_json(scored, debug_path)
        plan = GlobalCutPlanner(_planner_config()).plan(scored, duration_s=duration_s)
        lyrics_meta = {"enabled": lyrics_enabled, "provider": provider_name, "strict": strict,
                       "fallback_reason": fallback_reason, "word_count": len(timeline.words), "sentence_count": len(timeline.sentences),
                       "vad_region_count": len(timeline.vad_regions), "warnings": list(timeline.warnings), "timeline": timeline.to_dict()}
        boundary_meta = {
            "mode": mode, "actual_mode": actual_mode, "candidate_pool": pool, "candidate_debug_path": debug_path,
            "candidate_counts": {"acoustic": len(acoustic), "lyrics": len(lyrics), "lyrics_pooled": len(pooled), "beat": len(beats),
                                 "merged": len(merged), "total": len(scored), "selected": len(plan.selected_candidates),
                                 "suppressed": len(plan.suppressed_candidates), "lyrics_soft_prior": len(lyrics)},
            "planner": dict(plan.metadata),
            "selected": [c.to_dict() for c in plan.selected_candidates],
            "suppressed": [c.to_dict() for c in plan.suppressed_candidates],
        }
        return VPBDDetectionResult(list(plan.selected_candidates), plan, boundary_meta, lyrics_meta)

    # -- the ASR copy (reference `_write_asr_vocal_copy`, `:388-411`) --------------------------------------------
    def _asr_vocal_copy(self, state: Dict[str, Any], input_path: str, output_dir: str):
        """-> (path or None, int16 array or None).  The resident vocal stem as mono 16 kHz 16-bit PCM, in one kernel and one
        download (`Context.resample_poly_pcm16`: the resampler's floats go through the WAV writer's conversion without ever
        being stored; its saturation is the reference's `np.clip(-1, 1)`).  With an `output_dir` it is also written as
        `<stem of input_path>_vocal_for_asr.wav`.  Without device state (host-only callers) no copy is made."""
        hip, vocal = state.get("hip"), state.get("vocal")
        if hip is None or vocal is None:
            return None, None
        pcm16 = hip.resample_poly_pcm16(vocal, self.ASR_SAMPLE_RATE, self.sample_rate)
        if not output_dir:
            return None, pcm16
        from ..utils.audio_export import wav_header
        target = Path(output_dir)
        target.mkdir(parents=True, exist_ok=True)
        path = target / f"{Path(input_path).stem}_vocal_for_asr.wav"
        with open(path, "wb") as fh:
            fh.write(wav_header(int(pcm16.size), self.ASR_SAMPLE_RATE, 1, 2))
            fh.write(np.ascontiguousarray(pcm16, dtype="<i2").tobytes())
        return path, pcm16

    # -- pool members ---------------------------------------------------------------------------------------
    def _build_acoustic_candidates(self, *, vocal_track, original_audio, pure_vocal_detector, feature_cache, vad_segments,
                                   enable_mdd: bool, include_breath_candidates: bool = True, device_state=None) -> List[CutCandidate]:
        kwargs = {}
        if device_state and hasattr(pure_vocal_detector, "_context"):
            kwargs = {"vocal_dev": device_state.get("vocal"), "original_dev": device_state.get("mix")}
        pauses = pure_vocal_detector.detect_pure_vocal_pauses(
            vocal_track, enable_mdd_enhancement=enable_mdd, original_audio=original_audio, feature_cache=feature_cache,
            vad_segments=vad_segments, include_breath_candidates=include_breath_candidates, **kwargs)
        scale = float(_section("vpbd").get("breath_score_scale", 0.6)) if include_breath_candidates else 0.0
        raw = []
        for p in pauses or []:
            t = float(getattr(p, "cut_point", (p.start_time + p.end_time) / 2.0))
            meta = {"pause_start_s": float(getattr(p, "start_time", t)), "pause_end_s": float(getattr(p, "end_time", t)),
                    "pause_duration_s": float(getattr(p, "duration", 0.0))}
            if include_breath_candidates:
                meta["pause_type"] = str(getattr(p, "pause_type", ""))
            raw.append((t, float(getattr(p, "confidence", 1.0)), meta))
        return adapt_legacy_acoustic_candidates(raw, source=CandidateSource.ACOUSTIC_PAUSE, breath_score_scale=scale)

    def _build_beat_candidates(self, *, vocal_track, feature_cache, duration_s: float, device_state=None) -> List[CutCandidate]:
        cfg = _section("vpbd").get("beat_candidates", {})
        if not isinstance(cfg, dict) or not bool(cfg.get("enable", False)) or feature_cache is None:
            return []
        base = float(cfg.get("base_score", 0.3))
        if base <= 0.0:
            return []
        st = device_state or {}
        return generate_beat_candidates(
            beat_times=getattr(feature_cache, "beat_times", []), rms_series=getattr(feature_cache, "rms_series", []),
            hop_s=float(getattr(feature_cache, "hop_s", 0.0) or 0.0), duration_s=duration_s, sample_rate=self.sample_rate,
            vocal_track=vocal_track, bars_per_cut=int(cfg.get("bars_per_cut", 2)), base_score=base,
            hip=st.get("hip"), vocal_dev=st.get("vocal"))

    def _merge_candidate_pool(self, *groups: List[CutCandidate], tolerance_s: float = 0.12) -> List[CutCandidate]:
        ordered = sorted((c for g in groups for c in g), key=lambda c: (c.t, c.source.value))
        if not ordered:
            return []
        clusters: List[List[CutCandidate]] = [[ordered[0]]]
        for c in ordered[1:]:
            if c.t - clusters[-1][-1].t <= tolerance_s:
                clusters[-1].append(c)
            else:
                clusters.append([c])
        return [self._merge_cluster(cl) for cl in clusters]

    def _merge_cluster(self, cluster: List[CutCandidate]) -> CutCandidate:
        best = max(cluster, key=lambda c: c.score)
        reasons: List[str] = []
        sources: List[str] = []
        source_scores: Dict[str, float] = {}
        members: List[Dict[str, Any]] = []
        for c in cluster:
            for r in c.reasons:
                if r not in reasons:
                    reasons.append(r)
            s = c.source.value
            if s not in sources:
                sources.append(s)
            source_scores[s] = max(float(c.score), source_scores.get(s, 0.0))
            members.append({"t": c.t, "score": c.score, "source": s, "reasons": list(c.reasons)})
        meta = dict(best.meta)
        meta.update({"sources": sources, "source_count": len(sources), "source_scores": source_scores})
        if len(cluster) > 1:
            meta["merged_candidates"] = members
        return replace(best, reasons=reasons, meta=meta)

    # -- scoring ----------------------------------------------------------------------------------------------
    def _score_candidates(self, *, candidates: List[CutCandidate], timeline, feature_cache: Optional[Any]) -> List[CutCandidate]:
        beat_times = getattr(feature_cache, "beat_times", []) if feature_cache is not None else []
        rms_series = getattr(feature_cache, "rms_series", []) if feature_cache is not None else []
        hop_s = float(getattr(feature_cache, "hop_s", 0.0) or 0.0) if feature_cache is not None else 0.0
        extractor = BoundaryFeatureExtractor(
            timeline=timeline, beat_times=beat_times, mdd_times=self._mdd_valley_times(feature_cache), rms_series=rms_series,
            hop_s=hop_s, word_edge_tolerance_ms=float(_section("phrase_boundary").get("word_edge_tolerance_ms", 60.0)))
        scorer = PhraseBoundaryScorer.from_config(_section("phrase_boundary"))
        out: List[CutCandidate] = []
        for c in candidates:
            feats = extractor.extract(c.t, acoustic_pause=self._acoustic_pause_score(c))
            breath = self._breath_score(c)
            if breath > 0.0:
                feats = replace(feats, breath=breath)
            sc = scorer.score_candidate(c, feats)
            merged = dict(c.features)
            merged.update(sc.features)
            out.append(replace(sc, features=merged))
        return out

    @staticmethod
    def _acoustic_pause_score(c: CutCandidate) -> float:
        kinds = (CandidateSource.ACOUSTIC_PAUSE.value, CandidateSource.MDD_VALLEY.value)
        score = c.score if c.source.value in kinds else 0.0
        ss = c.meta.get("source_scores", {})
        if isinstance(ss, dict):
            for k in kinds:
                try:
                    score = max(score, float(ss.get(k, 0.0)))
                except (TypeError, ValueError):
                    continue
        return score

    @staticmethod
    def _breath_score(c: CutCandidate) -> float:
        score = c.score if c.source == CandidateSource.BREATH else 0.0
        ss = c.meta.get("source_scores", {})
        if isinstance(ss, dict):
            try:
                score = max(score, float(ss.get(CandidateSource.BREATH.value, 0.0)))
            except (TypeError, ValueError):
                pass
        return score

    @staticmethod
    def _mdd_valley_times(feature_cache: Optional[Any]) -> List[float]:
        """local minima of the cached MDD series at or below its 35th percentile (reference `:370-385`)."""
        if feature_cache is None:
            return []
        mdd = np.asarray(getattr(feature_cache, "mdd_series", []), dtype=np.float32)
        hop_s = float(getattr(feature_cache, "hop_s", 0.0) or 0.0)
        if mdd.size < 3 or hop_s <= 0.0:
            return []
        thr = float(np.percentile(mdd, 35))
        mid = mdd[1:-1].astype(np.float64)
        left = mdd[:-2].astype(np.float64); right = mdd[2:].astype(np.float64)
        hit = (mid <= thr) & ((mid < left) | (mid < right))
        return [(int(i) + 1) * hop_s for i in np.flatnonzero(hit)]


__all__ = ["VocalPhraseBoundaryDetector", "VPBDDetectionResult"]
