"""The hot-path slice of the reference's orchestrator: SURVEY.md §3.1 steps 2-9 of
`SeamlessSplitter._process_pure_vocal_split` (`src/vocal_smart_splitter/core/seamless_splitter.py:261-481`)
— separate -> feature cache -> pause detection -> pure-music spans + presence markers ->
`_finalize_and_filter_cuts_v2` -> integer `sample_boundaries` — for mode `v2.2_mdd` (and
`v2.1`, which only switches the MDD boost off, `:412`).

What follows in the reference (segment classification, layout refinement, local-valley refinement,
weak-tail merge, export; `:522-770`) is post-path policy and is out of scope this round
(SURVEY.md §8f "next" 1 and 4): `split_audio_seamlessly` returns the boundaries and the metadata
the manifest's `gpu` block needs, not exported files.

`_find_no_vocal_runs` (`:1706-1790`) and `_finalize_and_filter_cuts_v2` (`:1792-1879`) keep their
names and signatures; their RMS(2048/441) passes run on the stems resident in HBM.
"""
from __future__ import annotations

import dataclasses
import logging
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _native
from ..analysis.beat_analyzer import BeatAnalyzer, queue_frame_series
from ..analysis.chorus_regions import detect_chorus_regions
from ..analysis.features_cache import TrackFeatureCache, build_feature_cache
from .. import config as _config
from ..config import get_config
from ..config.auto_profile import (PROFILE_NAMES, apply_profile_overrides, build_auto_profile_overrides, build_style_weight_overrides,
                                   derive_alignment_overrides, derive_smart_cut_overrides, estimate_style, resolve_smart_cut_intent,
                                   should_apply_duration_overrides)
from ..cutting.refine import CutContext, CutPoint, CutRefineResult, finalize_cut_points
from ..detectors.pure_vocal_pause_detector import PureVocalPauseDetector, _bool_runs
from .enhanced_vocal_separator import EnhancedVocalSeparator, SeparationResult

logger = logging.getLogger(__name__)


def _fill_false_runs(mask: np.ndarray, max_len: int) -> np.ndarray:
    out = np.asarray(mask, dtype=bool).copy()
    for a, b, v in _bool_runs(out):
        if not v and (b - a) <= max_len:
            out[a:b] = True
    return out


def _remove_true_runs(mask: np.ndarray, max_len: int) -> np.ndarray:
    out = np.asarray(mask, dtype=bool).copy()
    for a, b, v in _bool_runs(out):
        if v and (b - a) <= max_len:
            out[a:b] = False
    return out


def host_vocal_coverage(mono: np.ndarray) -> float:
    """The reference's coverage formula on the host (`seamless_splitter.py:884-889`): the yardstick of `ac_abs_peak_coverage`."""
    mono = np.asarray(mono, dtype=np.float32)
    peak = float(np.max(np.abs(mono))) if mono.size else 0.0
    if peak <= 1e-9:
        return 0.0
    return float(np.mean(np.abs(mono) >= max(peak * 0.03, 1e-5)))


PRECISION_GUARD_AVG_MS = 150.0     # reference `seamless_splitter.py:66-67`
PRECISION_GUARD_P95_MS = 220.0


class SeamlessSplitter:
    SUPPORTED_MODES = ("v2.2_mdd", "v2.1", "vpbd_acoustic", "vpbd_asr", "librosa_onset", "hybrid_mdd", "vocal_separation")

    def __init__(self, sample_rate: int = 44100, *, separator: Optional[EnhancedVocalSeparator] = None,
                 device: Optional[str] = None) -> None:
        self.sample_rate = sample_rate
        self.separator = separator if separator is not None else EnhancedVocalSeparator(sample_rate, device=device)
        backend = getattr(self.separator, "_primary_backend", None)
        self._hip: Optional["_native.Context"] = getattr(backend, "hip", None)
        self.pure_vocal_detector = PureVocalPauseDetector(sample_rate, ctx=self._hip)
        from .vocal_phrase_boundary_detector import VocalPhraseBoundaryDetector
        self.vpbd_detector = VocalPhraseBoundaryDetector(sample_rate)
        self.beat_analyzer = BeatAnalyzer(sample_rate, ctx=self._hip)
        self._last_guard_adjustments_raw: list = []
        self._last_suppressed_cut_points: list = []
        self._last_auto_profile_meta: Optional[Dict] = None
        self._last_intent_meta: Optional[Dict] = None

    def _context(self) -> "_native.Context":
        if self._hip is None:
            self._hip = _native.Context()
        return self._hip

    # ------------------------------------------------------------------------------------------
    def split_track(self, original_audio: np.ndarray, mode: str = "v2.2_mdd", *, audio_dev=None, separation_gate=None,
                    unet_stream=None, beat_analysis: bool = False, hybrid_density: Optional[str] = None, input_path: str = "",
                    output_dir: str = "", smart_cut: Optional[bool] = None) -> Dict:
        """Steps 2-9 of SURVEY.md §3.1 on an in-memory mono float32 track at `sample_rate`.
        `separation_gate` (a lock shared by the workers of a `batch.TrackPipeline`) and `unet_stream` (the pipeline's one U-Net
        stream): with both, this track's separation is queued on that stream under the lock and the lock is released as soon as it is
        queued - the stream itself keeps the U-Nets of consecutive tracks one after the other, and the next one waits in the queue
        behind the running one.  With the gate alone (round 2's scheme) the lock is held until this track's U-Net has left the GPU and
        released before the host-bound tail.
        A planar stereo (2, N) track (and a [2, N] `audio_dev`) is separated on true L/R; detection, guards and boundaries run on its
        mono mix (L + R) * 0.5 exactly as on a mono track of those samples, and the result adds `vocal_track_stereo` /
        `instrumental_track_stereo` ([2, N]) and `mono_mix`.  Stereo tracks are not taken with a gate or U-Net stream.
        `beat_analysis=True` adds a `"beat_analysis"` block (tempo, bars, per-bar energy / centroid / bandwidth, high-energy and
        chorus bars: `_beat_analysis_block`) to the result of every mode that builds a feature cache - all but `librosa_onset`,
        which reports its own bar analysis, and `hybrid_mdd`, which always reports the one its cuts were taken from.  Off, nothing
        is launched for it.
        `hybrid_density` ("low" / "medium" / "high") overrides `hybrid_mdd.beat_cut_density` for a `hybrid_mdd` track.
        Mode `vocal_separation` separates and detects nothing: `_split_vocal_separation`.
        `input_path` / `output_dir` reach the VPBD detector as `input_path` / `asr_output_dir` and name nothing else (`vpbd_asr`: where the 16 kHz ASR copy of the vocal stem is written and
        what it is named after; empty: no file, the provider gets the samples only).
        `smart_cut`: the smart-cut intent and AutoProfile runtime (`_apply_smart_cut_runtime`) of a `vpbd_acoustic` / `vpbd_asr`
        track.  None (the default): it runs when the runtime configuration holds a `smart_cut.*` key as the call starts
        (`separate_and_segment(segments=, alignment=)` puts them there); True: it runs; False: it does not.  Where it does not run
        the track is split on the configuration as it stands.  Where it does, its overrides are applied between the feature cache
        and the detection, the result carries `intent` (and `auto_profile` for profile `auto`), and the runtime configuration is
        put back as it was found when the call returns or raises.  Not with a gate or a U-Net stream: the configuration is global
        to the process and the workers of a `batch.TrackPipeline` share it."""
        if mode not in self.SUPPORTED_MODES:
            raise NotImplementedError(f"mode {mode!r}: only the v2.2_mdd / v2.1 path is built this round")
        if original_audio is None or len(original_audio) == 0 or np.shape(original_audio)[-1] == 0:
            raise ValueError("split_track needs a non-empty mono track")
        if mode == "librosa_onset":
            if separation_gate is not None or unet_stream is not None:
                raise ValueError("librosa_onset tracks are split one at a time (no separation gate / U-Net stream)")
            return self._split_librosa_onset(original_audio, audio_dev)
        if mode == "vocal_separation":
            if separation_gate is not None or unet_stream is not None:
                raise ValueError("vocal_separation tracks are separated one at a time (no separation gate / U-Net stream)")
            if beat_analysis:
                raise ValueError("vocal_separation builds no feature cache: there is no beat analysis to report")
            return self._split_vocal_separation(original_audio, audio_dev)
        if mode == "hybrid_mdd":
            if separation_gate is not None or unet_stream is not None:
                raise ValueError("hybrid_mdd tracks are split one at a time (no separation gate / U-Net stream)")
            return self._split_hybrid_mdd(original_audio, audio_dev, hybrid_density)
        args = (original_audio, mode, audio_dev, separation_gate, unet_stream, beat_analysis, input_path, output_dir)
        if not self._smart_cut_active(mode, smart_cut):
            self._last_auto_profile_meta = self._last_intent_meta = None
            return self._split_pause_modes(*args, smart_cut=False)
        if separation_gate is not None or unet_stream is not None:
            raise ValueError("smart-cut tracks are split one at a time (no separation gate / U-Net stream): their overrides go "
                             "into the runtime configuration, which the workers of a pipeline share")
        saved = _config.snapshot()
        try:
            return self._split_pause_modes(*args, smart_cut=True)
        finally:
            _config.restore(saved)              # one track's profile never colours the next

    @staticmethod
    def _smart_cut_active(mode: str, smart_cut: Optional[bool]) -> bool:
        """Whether this track runs the smart-cut runtime: only a VPBD mode, and only when asked - by the flag, or by a `smart_cut`
        key among the runtime overrides.  (The reference runs it on every VPBD track)"""
        if mode not in ("vpbd_acoustic", "vpbd_asr"):
            if smart_cut:
                raise ValueError(f"smart_cut=True: mode {mode!r} has no smart-cut runtime (vpbd_acoustic / vpbd_asr have)")
            return False
        if smart_cut is not None:
            return bool(smart_cut)
        return any(k == "smart_cut" or k.startswith("smart_cut.") for k in _config.snapshot())

    def _split_pause_modes(self, original_audio: np.ndarray, mode: str, audio_dev, separation_gate, unet_stream, beat_analysis: bool,
                           input_path: str, output_dir: str, *, smart_cut: bool) -> Dict:
        """`split_track` for `v2.2_mdd`, `v2.1` and the VPBD modes, after its argument checks."""
        sr = self.sample_rate
        stereo = np.ndim(original_audio) == 2
        t0 = time.perf_counter()
        sep: SeparationResult = self.separator.separate_for_detection(original_audio, gpu_context=None, audio_dev=audio_dev,
                                                                     separation_gate=separation_gate, unet_stream=unet_stream)
        t_sep = time.perf_counter() - t0
        if stereo:
            original_audio = sep.mono_mix          # everything below reads the mono mix
        state = sep.device_state or {}
        vocal_track = sep.vocal_track
        cache: Optional[TrackFeatureCache] = sep.feature_cache
        if cache is None:
            cache = build_feature_cache(original_audio, vocal_track, sr, ctx=self._context(), mix_dev=state.get("mix"))
        beat_pending = self._beat_analysis_queue(original_audio, state) if beat_analysis else None
        markers = sep.quality_metrics or {}
        marker_times = [float(t) for t in markers.get("vocal_presence_cut_points_sec", []) if t is not None]

        t1 = time.perf_counter()
        is_vpbd = mode in {"vpbd_acoustic", "vpbd_asr"}
        result: Dict = {"success": True, "mode": mode, "gpu_meta": dict(sep.gpu_meta or {}),
                        "separation_confidence": sep.separation_confidence, "backend_used": sep.backend_used,
                        "vad_segments": sep.vad_segments, "feature_cache": cache,
                        "vocal_track": vocal_track, "instrumental_track": sep.instrumental_track, "device_state": state}
        if stereo:
            result.update({"vocal_track_stereo": sep.vocal_track_stereo, "instrumental_track_stereo": sep.instrumental_track_stereo,
                           "mono_mix": sep.mono_mix})
        if is_vpbd:
            # reference `:349`: intent, profile and duration overrides go into the runtime configuration ahead of the detection
            # (here only where asked for: `_smart_cut_active`); then `:362-408`
            auto_profile_meta = None
            if smart_cut:
                auto_profile_meta = self._apply_smart_cut_runtime(cache, vocal_track=vocal_track, vocal_dev=state.get("vocal"))
            vpbd = self.vpbd_detector.detect(mode=mode, vocal_track=vocal_track, original_audio=original_audio,
                                             pure_vocal_detector=self.pure_vocal_detector, feature_cache=cache,
                                             vad_segments=sep.vad_segments, input_path=input_path, asr_output_dir=output_dir,
                                             device_state=state)
            t_det = time.perf_counter() - t1
            cut_candidates = [(c.t, c.score) for c in vpbd.selected_candidates]
            rescue = [(c.t, c.score) for c in vpbd.planner_result.suppressed_candidates if float(c.score) > 0.0]
            if not cut_candidates and rescue:
                cut_candidates = rescue
            result.update({"boundary_detection": vpbd.boundary_detection, "lyrics_alignment": vpbd.lyrics_alignment,
                           "vpbd_selected_times": [c.t for c in vpbd.selected_candidates], "num_pauses": len(cut_candidates)})
            if not cut_candidates:
                result.update({"sample_boundaries": [0, len(original_audio)], "note": "no_vpbd_candidates",
                               "timings": {"separate_s": t_sep, "detect_s": t_det, "finalize_s": 0.0}})
                if auto_profile_meta is not None:       # `_create_single_segment_result` (`:2742-2744`) carries this block alone
                    result["auto_profile"] = auto_profile_meta
                result.update(self._single_segment_fields(vocal_track, len(original_audio), state.get("vocal")))
                self._beat_analysis_block(beat_pending, original_audio, cache, result)
                return result
            t2 = time.perf_counter()
        else:
            pauses = self.pure_vocal_detector.detect_pure_vocal_pauses(
                vocal_track, enable_mdd_enhancement=(mode == "v2.2_mdd"), original_audio=original_audio, feature_cache=cache,
                vad_segments=sep.vad_segments, vocal_dev=state.get("vocal"), original_dev=state.get("mix"))
            t_det = time.perf_counter() - t1
            result.update({"num_pauses": len(pauses), "pauses": pauses})
            if not pauses:      # `:421-433`: single segment
                result.update({"sample_boundaries": [0, len(original_audio)], "note": "no_pause_candidates",
                               "timings": {"separate_s": t_sep, "detect_s": t_det, "finalize_s": 0.0}})
                result.update(self._single_segment_fields(vocal_track, len(original_audio), state.get("vocal")))
                self._beat_analysis_block(beat_pending, original_audio, cache, result)
                return result
            t2 = time.perf_counter()
            cut_candidates = [(float(p.cut_point), float(p.confidence)) for p in pauses]
        min_pure_music = float(get_config("quality_control.pure_music_min_duration", 0.0))
        if min_pure_music > 0.0:
            for a, b in self._find_no_vocal_runs(vocal_track, min_pure_music, vocal_dev=state.get("vocal")):
                cut_candidates.append((float(a), 1.0))
                cut_candidates.append((float(b), 1.0))
        duration = len(original_audio) / sr
        protected = set()
        for t in marker_times:
            if t <= 0.0 or t >= duration:
                continue
            cut_candidates.append((t, 1.0))
            protected.add(int(round(t * sr)))
        refine = self._finalize_and_filter_cuts_v2(cut_candidates, original_audio, pure_vocal_audio=vocal_track,
                                                   mix_dev=state.get("mix"), vocal_dev=state.get("vocal"))
        self._last_suppressed_cut_points = list(refine.suppressed_points or [])
        bounds = sorted(set(refine.sample_boundaries))
        lyrics = vpbd.lyrics_alignment if is_vpbd and mode == "vpbd_asr" else None
        if lyrics is not None:      # `:484-493`: a guard move from outside a word into one is undone
            bounds, restored = self._restore_guard_points_outside_lyrics_words(
                bounds, self._last_guard_adjustments_raw, self._collect_lyrics_word_intervals(lyrics),
                sample_count=len(original_audio), min_gap_s=float(get_config("quality_control.min_split_gap", 1.0)))
            if restored is not None:
                self._last_guard_adjustments_raw = list(restored)
        if is_vpbd:         # `:494-499`: the planner block records where the guards moved each selected candidate
            from ..cutting.global_cut_planner import apply_guard_shift_metadata
            vpbd.boundary_detection["planner"] = dict(apply_guard_shift_metadata(vpbd.planner_result, self._last_guard_adjustments_raw).metadata)
        if protected:       # `:501-508`
            total = len(original_audio)
            aug = set(int(b) for b in bounds)
            for s in protected:
                s = int(min(max(s, 0), total))
                if s not in (0, total):
                    aug.add(s)
            bounds = sorted(aug)
        t_fin = time.perf_counter() - t2
        t3 = time.perf_counter()
        policy = self._apply_boundary_policy(bounds, vocal_track, len(original_audio), cache, vocal_dev=state.get("vocal"),
                                             lyrics_alignment=lyrics)
        result.update(policy)
        if mode == "vpbd_asr":
            result["lyrics_cut_protection_applied"] = False         # `:658,767`: the reference reports the switch and never sets it
        result["timings_policy_s"] = time.perf_counter() - t3
        kept = list(self._last_guard_adjustments_raw)               # after the layout refiner's filter (`:602`)
        stats = self._guard_shift_stats(kept)
        result.update({"sample_boundaries": bounds, "refine_boundaries": list(refine.sample_boundaries),
                       "cut_candidates": cut_candidates,
                       "guard_adjustments": kept, "guard_adjustments_unfiltered": list(refine.adjustments or []),
                       "guard_shift_stats": stats,
                       "precision_guard_ok": bool(stats["avg_shift_ms"] <= PRECISION_GUARD_AVG_MS and stats["p95_shift_ms"] <= PRECISION_GUARD_P95_MS),
                       "precision_guard_threshold_ms": {"avg": PRECISION_GUARD_AVG_MS, "p95": PRECISION_GUARD_P95_MS},
                       "timings": {"separate_s": t_sep, "detect_s": t_det, "finalize_s": t_fin}})
        if is_vpbd and smart_cut:           # `:761-765`
            if auto_profile_meta is not None:
                result["auto_profile"] = auto_profile_meta
            if self._last_intent_meta is not None:
                result["intent"] = dict(self._last_intent_meta)
        self._beat_analysis_block(beat_pending, original_audio, cache, result)
        return result

    # ---- smart-cut intent and AutoProfile (reference `seamless_splitter.py:772-893`) ----------------------------------
    COVERAGE_ON_DEVICE = True           # the vocal coverage of a resident stem comes from `ac_abs_peak_coverage`

    def _apply_smart_cut_runtime(self, feature_cache: Optional[TrackFeatureCache], *, vocal_track: Optional[np.ndarray] = None,
                                 vocal_dev=None) -> Optional[Dict]:
        """The `smart_cut` section -> runtime overrides, written in one `set_runtime_config` ahead of the boundary detection:
        the intent (with the keys the caller set on purpose), the duration knobs where the intent moves them, the profile
        (`auto`: vocal coverage -> `estimate_style` -> the blended profile; a name; an unknown one: pop, with a warning), and on
        top of the profile's phrase weights the alignment.  -> the AutoProfile record (None for a named profile); it and the
        intent record are kept in `_last_auto_profile_meta` / `_last_intent_meta`."""
        smart_cfg = get_config("smart_cut", {}) or {}
        if not isinstance(smart_cfg, dict):
            smart_cfg = {}
        stated = _config.get_runtime_override_keys()
        intent = resolve_smart_cut_intent(smart_cfg, explicit_keys=stated)
        profile = str(intent.get("profile", "auto") or "auto").strip().lower()
        overrides: Dict = {}
        if should_apply_duration_overrides(smart_cfg, explicit_keys=stated):
            overrides.update(derive_smart_cut_overrides(smart_cfg, explicit_keys=stated))
        auto_meta: Optional[Dict] = None
        if profile == "auto":
            self._attach_vocal_coverage(feature_cache, vocal_track, vocal_dev=vocal_dev)
            picked = build_auto_profile_overrides(estimate_style(feature_cache), cut_style="natural")
            auto_meta = dict(picked.get("meta.auto_profile", {}))
            overrides.update(picked)
            logger.info("[AutoProfile] style=%s confidence=%.3f bpm=%s alignment=%s", auto_meta.get("style"),
                        float(auto_meta.get("confidence") or 0.0), auto_meta.get("bpm"), intent.get("alignment"))
        else:
            if profile not in PROFILE_NAMES:
                logger.warning("[AutoProfile] unknown smart_cut.profile=%s; falling back to pop", profile)
                profile = "pop"
            overrides.update(apply_profile_overrides(profile))
            overrides.update(build_style_weight_overrides(profile, cut_style="natural"))
            overrides["meta.profile"] = profile
        by_alignment = derive_alignment_overrides(intent.get("alignment", 0.5), self._phrase_weights_from_overrides(overrides),
                                                  alignment_poles=get_config("phrase_boundary.alignment_poles", None))
        overrides.update(by_alignment)
        intent = dict(intent)
        intent["applied_overrides"] = sorted(k for k in by_alignment if not k.startswith("meta."))
        if auto_meta is not None:
            auto_meta["alignment"] = {"value": intent.get("alignment"), "raw": intent.get("alignment_raw")}
        overrides["meta.intent"] = intent
        _config.set_runtime_config(overrides)
        self._last_auto_profile_meta = auto_meta
        self._last_intent_meta = intent
        return auto_meta

    @staticmethod
    def _phrase_weights_from_overrides(overrides: Dict) -> Dict[str, float]:
        """The eight phrase-boundary weights as the profile left them: from `overrides`, else from the configuration."""
        from ..config.auto_profile import WEIGHT_KEYS
        flat = {k: f"phrase_boundary.weights.{k}" for k in WEIGHT_KEYS}
        return {k: float(overrides[f]) if f in overrides else float(get_config(f, 0.0)) for k, f in flat.items()}

    def _attach_vocal_coverage(self, feature_cache: Optional[TrackFeatureCache], vocal_track: Optional[np.ndarray], *,
                               vocal_dev=None) -> None:
        """`feature_cache.vocal_coverage_ratio` = the share of the vocal stem's samples at or above max(3 % of its peak, 1e-5), 0.0 for
        a stem whose peak is at most 1e-9 (`:873-893`).  Nothing without a cache or a stem, for an empty stem, or where the cache
        carries the ratio already.  A mono stem resident on the device is swept there (`Context.vocal_coverage`: exact peak and
        count, 16 bytes downloaded); otherwise the host formula.  The attribute is set beside the dataclass's fields, as the
        reference does: a `dataclasses.replace` copy of the cache does not carry it."""
        if feature_cache is None or hasattr(feature_cache, "vocal_coverage_ratio"):
            return
        if self.COVERAGE_ON_DEVICE and vocal_dev is not None and vocal_dev.dim() == 1:
            n = int(vocal_dev.numel())
            if n == 0:
                return
            peak, _, count = self._context().vocal_coverage(vocal_dev)
            coverage = _native.coverage_from(peak, count, n)
        elif vocal_track is not None:
            audio = np.asarray(vocal_track, dtype=np.float32)
            if audio.size == 0:
                return
            coverage = host_vocal_coverage(audio if audio.ndim == 1 else np.mean(audio, axis=-1))
        else:
            return
        setattr(feature_cache, "vocal_coverage_ratio", max(0.0, min(1.0, coverage)))

    # ---- mode `vocal_separation`: the two stems and nothing else (reference `seamless_splitter.py:958-1036`) ----------
    def _split_vocal_separation(self, original_audio: np.ndarray, audio_dev=None) -> Dict:
        """`_process_vocal_separation_only` on an in-memory track: separate, and report the reference's result fields (`:1012-1035`)
        with no segments and no cuts.  The stems come back as finished PCM_24 bytes (`stem_pcm24`, `separate_only`); the caller
        writes them (`api._split_and_export`)."""
        t0 = time.perf_counter()
        sep: SeparationResult = self.separator.separate_only(original_audio, gpu_context=None, audio_dev=audio_dev)
        return {"success": True, "mode": "vocal_separation", "method": "vocal_separation_only", "num_segments": 0,
                "segment_durations": [], "stem_pcm24": sep.stem_pcm24, "backend_used": sep.backend_used,
                "separation_confidence": sep.separation_confidence, "guard_shift_stats": self._guard_shift_stats([]),
                "precision_guard_ok": True, "precision_guard_threshold_ms": {"avg": PRECISION_GUARD_AVG_MS, "p95": PRECISION_GUARD_P95_MS},
                "gpu_meta": dict(sep.gpu_meta or {}), "timings": {"separate_s": time.perf_counter() - t0}}

    # ---- optional beat / bar analysis block (reference `audio_cut.analysis.beat_analyzer`, `chorus_regions`) -----------
    def _beat_analysis_queue(self, mono_mix: np.ndarray, state: Dict, hop_length: Optional[int] = None):
        """Queue the RMS and centroid / bandwidth passes over the resident mix on a stream of their own, right after the
        separation: they run beside the detection tail, which is bound by the host, instead of in front of it."""
        import torch
        hip = state.get("hip") or self._context()
        mix_dev = state.get("mix")
        if mix_dev is None:
            mix_dev = hip.to_device(np.ascontiguousarray(mono_mix, dtype=np.float32))
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=hip.device)
        side.wait_stream(main)                                  # the mix is written on the main stream
        with torch.cuda.stream(side):
            series = queue_frame_series(hip, mix_dev, self.sample_rate, hop_length or self.beat_analyzer.hop_length)
            done = torch.cuda.Event()
            done.record()
        mix_dev.record_stream(side)
        for t in series:
            t.record_stream(main)                               # allocated on the side stream, read by `ac_bar_means3` on the main one
        return hip, mix_dev, series, done

    def _beat_analysis_block(self, pending, mono_mix: np.ndarray, cache: TrackFeatureCache, result: Dict) -> None:
        """`result["beat_analysis"]`: `BeatAnalyzer.analyze` on the mix with the cache's beats and BPM, and the chorus bars of the
        spectral-fusion `detect_chorus_regions` over its per-bar lists."""
        if pending is None:
            return
        import torch
        hip, mix_dev, series, done = pending
        torch.cuda.current_stream().wait_event(done)
        res = self.beat_analyzer.analyze(mono_mix, sr=self.sample_rate, feature_cache=cache, ctx=hip, audio_dev=mix_dev,
                                         frame_series=series)
        chorus = detect_chorus_regions(res.bar_energies, res.energy_threshold, bar_centroids=res.bar_spectral_centroids,
                                       bar_bandwidths=res.bar_spectral_bandwidths)
        result["beat_analysis"] = {"tempo": res.tempo, "bar_times": [float(t) for t in res.bar_times],
                                   "bar_duration": res.bar_duration, "bar_energies": list(res.bar_energies),
                                   "bar_spectral_centroids": list(res.bar_spectral_centroids),
                                   "bar_spectral_bandwidths": list(res.bar_spectral_bandwidths),
                                   "energy_threshold": res.energy_threshold, "high_energy_bars": sorted(res.high_energy_bars),
                                   "chorus_bars": sorted(chorus)}

    @staticmethod
    def _guard_shift_stats(adjustments: Sequence) -> Dict[str, float]:
        """`_set_guard_adjustments` (`:2423-2470`): how far the quiet guards moved the kept cuts, in ms."""
        total = np.array([a.final_shift_ms for a in adjustments], dtype=float)
        if total.size == 0:
            return {"avg_shift_ms": 0.0, "max_shift_ms": 0.0, "avg_guard_only_shift_ms": 0.0, "avg_vocal_guard_shift_ms": 0.0,
                    "avg_mix_guard_shift_ms": 0.0, "p95_shift_ms": 0.0, "count": 0}
        vocal = np.array([a.guard_shift_ms for a in adjustments], dtype=float)
        mean_pos = lambda v: float(sum(x for x in v.tolist() if x > 0) / max(1, int((v > 0).sum()))) if (v > 0).any() else 0.0
        return {"avg_shift_ms": float(sum(abs(x) for x in total.tolist()) / total.size), "max_shift_ms": float(np.abs(total).max()),
                "avg_guard_only_shift_ms": mean_pos(total), "avg_vocal_guard_shift_ms": mean_pos(vocal),
                "avg_mix_guard_shift_ms": mean_pos(total - vocal), "p95_shift_ms": float(np.percentile(np.abs(total), 95.0)),
                "count": int(total.size)}

    # ---- mode `librosa_onset`: bar-aligned smart segmentation (reference `seamless_splitter.py:1038-1349`) -----------
    def _split_librosa_onset(self, original_audio: np.ndarray, audio_dev=None) -> Dict:
        """Steps 0-7 and 9 of `_process_librosa_onset_split` on an in-memory track: (separation) -> tempo -> bar grid -> mean RMS
        per bar and silent frames (`ac_bar_energy_silence`) -> chorus / verse bars -> density-controlled bar cuts with forced
        cuts at silences -> sample points -> human / music labels from both stems (`ac_segment_pair_energy`).
        The mix is read once for the RMS(2048, hop) series, which is queued before the tempo is known; the tempo is the only
        host decision between that pass and the bar kernel.  A track whose tempo comes out 0 makes the reference divide by
        zero and report `{'success': False}` (`:1097`, `:231-233`): so does this."""
        from ..analysis.rhythm import beat_track_from_device
        from ..config import get_librosa_onset_config
        from ..cutting import smart_segment as SS
        import torch
        sr = self.sample_rate
        lo_config = get_librosa_onset_config()
        use_vocal = bool(lo_config["use_vocal_separation"])
        stereo = np.ndim(original_audio) == 2
        n = int(np.shape(original_audio)[-1])
        duration = n / float(sr)
        t0 = time.perf_counter()
        sep: Optional[SeparationResult] = None
        if use_vocal:
            sep = self.separator.separate_for_detection(original_audio, gpu_context=None, audio_dev=audio_dev)
            state = dict(sep.device_state or {})
            hip = state.get("hip") or self._context()
        else:                                   # no U-Net: the track goes to the device for the analysis alone
            hip = self._context()
            track_dev = audio_dev if audio_dev is not None else hip.to_device(np.ascontiguousarray(original_audio, dtype=np.float32))
            state = {"hip": hip, "mix": torch.add(track_dev[0], track_dev[1]).mul_(0.5) if stereo else track_dev}
            if stereo:
                state["mix_stereo"] = track_dev
        mix_dev = state.get("mix")
        if mix_dev is None:
            mono = sep.mono_mix if stereo else original_audio
            mix_dev = hip.to_device(np.ascontiguousarray(mono, dtype=np.float32))
            state["mix"] = mix_dev
        t_sep = time.perf_counter() - t0

        # 3. features (`:1089-1165`)
        t1 = time.perf_counter()
        hop = int(lo_config["energy_analysis"].get("hop_length", 512))
        time_signature = lo_config["beat"].get("time_signature", 4)
        rms_dev = hip.frame_rms(mix_dev, 2048, hop)                        # the one pass over the mix, queued ahead of the tempo
        _, mel = hip.stft2048_features(mix_dev, hop, want_flat=False, want_mel=True)
        env_dev = hip.onset_strength(mel, hop, "median")                    # librosa.beat.beat_track's envelope
        del mel
        tempo, beats, _ = beat_track_from_device(hip, env_dev, sr, hop)
        result: Dict = {"mode": "librosa_onset", "method": "smart_segment_v2", "use_vocal_preprocessing": use_vocal,
                        "gpu_meta": dict(sep.gpu_meta or {}) if sep is not None else {},
                        "separation_confidence": sep.separation_confidence if sep is not None else None,
                        "backend_used": sep.backend_used if sep is not None else None, "device_state": state,
                        "vocal_track": sep.vocal_track if sep is not None else None,
                        "instrumental_track": sep.instrumental_track if sep is not None else None}
        if stereo and sep is not None:
            result.update({"vocal_track_stereo": sep.vocal_track_stereo, "instrumental_track_stereo": sep.instrumental_track_stereo,
                           "mono_mix": sep.mono_mix})
        try:
            bar_duration = 60.0 / tempo * time_signature
        except ZeroDivisionError as exc:
            logger.error("split failed: %s", exc)
            result.update({"success": False, "error": str(exc), "bpm": tempo})
            return result
        n_frames = int(rms_dev.numel())
        rms_times = SS.rms_frame_times(n_frames, sr, hop)
        bar_times = SS.bar_grid(duration, bar_duration)
        bar_lo, bar_hi = SS.bar_frame_ranges(rms_times, bar_times)
        silence_cfg = lo_config["silence"]
        means, silent = hip.bar_energy_silence(rms_dev, bar_lo, bar_hi, float(silence_cfg["threshold_db"]))
        bar_energies = [float(e) for e in means]
        energy_cfg = lo_config["energy_analysis"]
        bar_types, thr_chorus, thr_peak = SS.classify_bars(bar_energies, energy_cfg.get("chorus_percentile", 60),
                                                           energy_cfg.get("chorus_peak_percentile", 80))
        silences = SS.silence_boundaries(silent, rms_times, duration, silence_cfg["min_duration"])

        # 4.-6. density, cut times, sample points (`:1167-1250`)
        density_cfg = SS.density_config(lo_config)
        cut_times = SS.plan_bar_cuts(bar_times, bar_types, silences, density_cfg, duration,
                                     float(get_config("segment_layout.soft_min_s", 2.0)))
        cuts = SS.to_sample_points(cut_times, sr, n)
        t_det = time.perf_counter() - t1

        # 7. human / music labels (`:1252-1273`)
        t2 = time.perf_counter()
        vocal_dev = state.get("vocal") if (sep is not None and sep.vocal_track is not None) else None
        if sep is not None and sep.vocal_track is not None and vocal_dev is None:
            vocal_dev = hip.to_device(np.ascontiguousarray(sep.vocal_track, dtype=np.float32))
        vocal_ss = inst_ss = None
        if vocal_dev is not None:
            inst_dev = None
            if sep.instrumental_track is not None:
                inst_dev = state.get("instrumental")
                if inst_dev is None:
                    inst_dev = hip.to_device(np.ascontiguousarray(sep.instrumental_track, dtype=np.float32))
            vocal_ss, inst_ss = hip.segment_pair_energy(vocal_dev, inst_dev, cuts[:-1], cuts[1:])
            if inst_dev is None:
                inst_ss = None
        flags = SS.label_segments(vocal_ss, inst_ss, cuts)
        # `:1282`: the sample-level split glues a slice under 10 ms to its neighbour.  As in the reference the cut points then
        # keep the glued point while flags and spans do not; the soft_min_s merge above leaves no such slice unless it is
        # configured under 10 ms.
        spans, merged_flags = self._sample_level_spans(n, cuts, flags)
        spans = list(spans)
        t_fin = time.perf_counter() - t2
        result.update({"success": True, "bpm": tempo, "bar_duration_s": bar_duration, "density": lo_config["density"],
                       "silence_boundaries": silences, "bar_energies": bar_energies, "bar_types": bar_types,
                       "sample_boundaries": list(cuts), "cuts_samples": list(cuts),
                       "cuts_sec": [c / float(sr) for c in cuts], "segment_vocal_flags": list(merged_flags or []),
                       "segment_spans": spans, "segment_durations": [(hi - lo) / float(sr) for lo, hi in spans],
                       "segment_layout_applied": False, "precision_guard_ok": True,
                       "timings": {"separate_s": t_sep, "detect_s": t_det, "finalize_s": t_fin}})
        return result

    # ---- mode `hybrid_mdd`: phrase-pause cuts snapped to beats in chorus bars (reference `seamless_splitter.py:1351-1704`) -----------
    def _hybrid_mdd_base(self, original_audio: np.ndarray, audio_dev=None) -> Dict:
        """The `v2.2_mdd` result `hybrid_mdd` builds on: its `cuts_samples` are the MDD cut points, and its stems, feature cache
        and device state are reused - ONE separation, where the reference separates for the stems and again inside its MDD run."""
        return self.split_track(original_audio, "v2.2_mdd", audio_dev=audio_dev)

    def _quiet_gate(self, hip, gate_dev, times: Sequence[float], guard_win_ms: float, guard_db: float) -> Dict:
        """`is_quiet_vocal_window` (`strategies/base.py:160-200`) for all of `times` at once: one `ac_quiet_gate_meansq` launch over
        the resident stem, one download.  -> the decisions by centre sample, and the numbers they were taken on."""
        from ..cutting import hybrid_strategies as HS
        sr = self.sample_rate
        half_win = HS.gate_half_window(sr, guard_win_ms)
        centers = sorted({HS.gate_center(float(t), sr) for t in times})
        block_ms, point_ms, count = hip.quiet_gate(gate_dev, half_win, np.asarray(centers, dtype=np.int64))
        floor_db, point_db, quiet = HS.gate_decisions(block_ms, point_ms, count, guard_db)
        return {"half_win": half_win, "floor_db": floor_db, "centers": centers, "point_db": [float(v) for v in point_db],
                "point_count": [int(c) for c in count], "quiet": {c: bool(q) for c, q in zip(centers, quiet)}}

    @staticmethod
    def _remap_lib_flags_to_refined_cuts(raw_cut_points: Sequence[int], raw_lib_flags: Sequence[bool],
                                         refined_cut_points: Sequence[int]) -> List[bool]:
        """`:2485-2513`: a refined segment takes the flag of the raw segment whose END is nearest to its own end; a segment that
        ends at the end of the track, or whose nearest raw end is the end of the track, is never `_lib`."""
        raw_points = list(raw_cut_points)
        refined_points = list(refined_cut_points)
        if len(refined_points) < 2:
            return []
        if len(raw_points) < 2:
            return [False] * (len(refined_points) - 1)
        raw_end_flags = []
        for idx, raw_end in enumerate(raw_points[1:]):
            raw_end_flags.append((int(raw_end), bool(raw_lib_flags[idx]) if idx < len(raw_lib_flags) else False))
        remapped: List[bool] = []
        for refined_end in refined_points[1:]:
            nearest_raw_end, nearest_flag = min(raw_end_flags, key=lambda item: abs(int(refined_end) - item[0]))
            if int(refined_end) == raw_points[-1] or nearest_raw_end == raw_points[-1]:
                remapped.append(False)
            else:
                remapped.append(nearest_flag)
        return remapped

    def _hybrid_micro_merge(self, cut_points: Sequence[int], lib_flags: Sequence[bool], micro_merge_s: float):
        """`:1512-1560`: a segment shorter than `micro_merge_s` that is neither the last one nor `_lib` joins the segment after
        it, and the run it joins loses its flag.  -> (cut points, flags), the inputs themselves when nothing merged."""
        final_cut_points, lib_cut_flags = list(cut_points), list(lib_flags)
        if not (micro_merge_s > 0 and len(final_cut_points) > 2):
            return final_cut_points, lib_cut_flags
        merged_cut_points: List[int] = [final_cut_points[0]]
        merged_lib_flags: List[bool] = []
        current_segment_was_merged = False
        for i in range(len(final_cut_points) - 1):
            duration_s = (final_cut_points[i + 1] - final_cut_points[i]) / float(self.sample_rate)
            is_lib_segment = lib_cut_flags[i] if i < len(lib_cut_flags) else False
            if duration_s < micro_merge_s and i < len(final_cut_points) - 2 and not is_lib_segment:
                current_segment_was_merged = True
            else:
                merged_cut_points.append(final_cut_points[i + 1])
                if current_segment_was_merged:
                    merged_lib_flags.append(False)
                elif i < len(lib_cut_flags):
                    merged_lib_flags.append(lib_cut_flags[i])
                else:
                    merged_lib_flags.append(False)
                current_segment_was_merged = False
        if len(merged_cut_points) != len(final_cut_points):
            return merged_cut_points, merged_lib_flags
        return final_cut_points, lib_cut_flags

    def _split_hybrid_mdd(self, original_audio: np.ndarray, audio_dev=None, density_override: Optional[str] = None) -> Dict:
        """`_process_hybrid_mdd_split` on an in-memory track: MDD cut points (`_hybrid_mdd_base`) -> beat / bar analysis of the
        mix -> quiet gate of every beat and bar line on the vocal stem (one launch) -> strategy (`snap_to_beat` / `beat_only`)
        -> quiet guards on the interior cuts -> `_lib` flags remapped to the guarded cuts -> human / music labels -> micro-merge
        -> sample-level spans."""
        from ..config import get_hybrid_mdd_config
        from ..cutting import hybrid_strategies as HS
        sr = self.sample_rate
        hybrid_config = get_hybrid_mdd_config(density_override)
        energy_percentile = hybrid_config["energy_percentile"]
        bars_per_cut = hybrid_config["bars_per_cut"]
        beat_cfg = hybrid_config["beat_detection"]
        snap_tolerance_ms = hybrid_config["snap_tolerance_ms"]
        vad_protection = hybrid_config["vad_protection"]
        chorus_force_snap = bool(hybrid_config.get("chorus_force_snap", False))
        guard_db = float(get_config("quality_control.enforce_quiet_cut.guard_db", 2.5))
        guard_win_ms = float(get_config("quality_control.enforce_quiet_cut.win_ms", 80))
        lib_alignment = hybrid_config.get("lib_alignment", "snap_to_beat")
        stereo = np.ndim(original_audio) == 2

        t0 = time.perf_counter()
        base = self._hybrid_mdd_base(original_audio, audio_dev)
        t_base = time.perf_counter() - t0
        if base.get("success"):
            mdd_cut_points_samples = [int(c) for c in base.get("cuts_samples", [])]
        else:                                               # `:1416-1424`
            if lib_alignment == "snap_to_beat":
                logger.warning("[HYBRID_MDD] MDD failed for snap_to_beat; fallback to beat_only")
                lib_alignment = "beat_only"
            if lib_alignment == "beat_only":
                mdd_cut_points_samples = []
            else:
                return base
        t1 = time.perf_counter()
        if stereo:
            mono = base.get("mono_mix")
            if mono is None:
                mono = (original_audio[0] + original_audio[1]) * np.float32(0.5)
        else:
            mono = original_audio
        state = dict(base.get("device_state") or {})
        hip = state.get("hip") or self._context()
        n = len(mono)
        if state.get("mix") is None:
            state["mix"] = hip.to_device(np.ascontiguousarray(mono, dtype=np.float32))
        stem = base.get("vocal_track")
        vocal_track = stem if stem is not None else mono       # `:1403`: the guards and labels read the mix without a stem
        vocal_dev = state.get("vocal") if stem is not None else state["mix"]
        if vocal_dev is None:
            vocal_dev = hip.to_device(np.ascontiguousarray(vocal_track, dtype=np.float32))
        cache = base.get("feature_cache")

        pending = self._beat_analysis_queue(mono, state, int(beat_cfg["hop_length"]))
        import torch
        _, mix_dev, series, done = pending
        torch.cuda.current_stream().wait_event(done)
        beat_result = self.beat_analyzer.analyze(mono, sr=sr, hop_length=beat_cfg["hop_length"], time_signature=beat_cfg["time_signature"],
                                                 energy_percentile=energy_percentile, feature_cache=cache, ctx=hip, audio_dev=mix_dev,
                                                 frame_series=series)
        gate = self._quiet_gate(hip, vocal_dev, [float(t) for t in beat_result.beat_times] + [float(t) for t in beat_result.bar_times],
                                guard_win_ms, guard_db)

        min_segment_s = float((get_config("segment_layout", {}) or {}).get("soft_min_s", 2.0))
        micro_merge_s = float((get_config("segment_layout", {}) or {}).get("micro_merge_s", 2.0))
        context = HS.SegmentationContext(
            audio=mono, sample_rate=sr, tempo=beat_result.tempo, beat_times=beat_result.beat_times, bar_times=beat_result.bar_times,
            bar_duration=beat_result.bar_duration, mdd_cut_points_samples=mdd_cut_points_samples,
            energy_threshold=beat_result.energy_threshold, bar_energies=beat_result.bar_energies,
            bar_spectral_centroids=beat_result.bar_spectral_centroids, bar_spectral_bandwidths=beat_result.bar_spectral_bandwidths,
            quiet_gate=gate["quiet"],
            config={"density": hybrid_config["density"], "enable_beat_cuts": hybrid_config["enable_beat_cuts"],
                    "bars_per_cut": bars_per_cut, "min_segment_s": min_segment_s, "energy_percentile": energy_percentile,
                    "snap_to_pause_ms": beat_cfg["snap_to_pause_ms"], "snap_tolerance_ms": snap_tolerance_ms,
                    "vad_protection": vad_protection, "chorus_force_snap": chorus_force_snap, "guard_db": guard_db,
                    "guard_win_ms": guard_win_ms})
        strategies = {"beat_only": HS.BeatOnlyStrategy(), "snap_to_beat": HS.SnapToBeatStrategy()}
        strategy = strategies.get(lib_alignment)
        if strategy is None:
            logger.warning("[HYBRID_MDD] Unknown lib_alignment=%s, fallback to snap_to_beat", lib_alignment)
            lib_alignment = "snap_to_beat"
            strategy = strategies[lib_alignment]
        seg_result = strategy.generate_cut_points(context)
        final_cut_points = list(seg_result.cut_points_samples)
        lib_cut_flags = list(seg_result.lib_flags)
        t_det = time.perf_counter() - t1

        t2 = time.perf_counter()
        raw_strategy_cut_points, raw_strategy_lib_flags = list(final_cut_points), list(lib_cut_flags)
        self._last_guard_adjustments_raw = []               # the guard statistics below are this mode's, not the MDD run's
        self._last_suppressed_cut_points = []
        if len(raw_strategy_cut_points) > 2:
            refined = self._finalize_and_filter_cuts_v2([(s / float(sr), 1.0) for s in raw_strategy_cut_points[1:-1]], mono,
                                                        pure_vocal_audio=vocal_track, mix_dev=state["mix"], vocal_dev=vocal_dev)
            self._last_suppressed_cut_points = list(refined.suppressed_points or [])
            guarded_cut_points = [int(b) for b in refined.sample_boundaries]
            if len(guarded_cut_points) >= 2:
                final_cut_points = guarded_cut_points
                lib_cut_flags = self._remap_lib_flags_to_refined_cuts(raw_strategy_cut_points, raw_strategy_lib_flags, final_cut_points)
        refined_cut_points, refined_lib_flags = list(final_cut_points), list(lib_cut_flags)
        segment_vocal_flags = self._classify_segments_vocal_presence(vocal_track, final_cut_points, vocal_dev=vocal_dev)
        merged_points, merged_flags = self._hybrid_micro_merge(final_cut_points, lib_cut_flags, micro_merge_s)
        if len(merged_points) != len(final_cut_points):
            final_cut_points, lib_cut_flags = merged_points, merged_flags
            segment_vocal_flags = self._classify_segments_vocal_presence(vocal_track, final_cut_points, vocal_dev=vocal_dev)
        spans, returned_flags = self._sample_level_spans(n, final_cut_points, segment_vocal_flags)
        spans = list(spans)
        t_fin = time.perf_counter() - t2

        kept = list(self._last_guard_adjustments_raw)
        stats = self._guard_shift_stats(kept)
        t_sep = float((base.get("timings") or {}).get("separate_s", 0.0))
        if lib_alignment == "beat_only":
            hybrid_meta = {"density": hybrid_config["density"], "lib_alignment": "beat_only", "bars_per_cut": bars_per_cut}
            strategy_metadata = {"vad_blocked": seg_result.metadata["vad_blocked"]}
        else:
            hybrid_meta = {"density": hybrid_config["density"], "lib_alignment": "snap_to_beat", "bars_per_cut": bars_per_cut,
                           "snap_tolerance_ms": snap_tolerance_ms, "vad_protection": vad_protection}
            strategy_metadata = {"snap_stats": dict(seg_result.metadata["snap_stats"])}
        result: Dict = {
            "success": True, "mode": "hybrid_mdd", "method": f"hybrid_mdd_{lib_alignment}", "strategy": lib_alignment,
            "gpu_meta": dict(base.get("gpu_meta") or {}), "separation_confidence": base.get("separation_confidence"),
            "backend_used": base.get("backend_used"), "vad_segments": base.get("vad_segments"), "feature_cache": cache,
            "vocal_track": stem, "instrumental_track": base.get("instrumental_track"), "device_state": state,
            "mdd_success": bool(base.get("success")), "mdd_cut_points_samples": list(mdd_cut_points_samples),
            "strategy_cut_points_samples": raw_strategy_cut_points, "strategy_lib_flags": raw_strategy_lib_flags,
            "sample_boundaries": refined_cut_points, "refined_lib_flags": refined_lib_flags,
            "cuts_samples": list(final_cut_points), "cuts_sec": [c / float(sr) for c in final_cut_points],
            "segment_vocal_flags": list(returned_flags if returned_flags else segment_vocal_flags),
            "segment_spans": spans, "segment_durations": [(hi - lo) / float(sr) for lo, hi in spans],
            "segment_lib_flags": list(lib_cut_flags), "lib_segment_count": sum(1 for f in lib_cut_flags if f),
            "lib_suffix": hybrid_config["labeling"]["lib_suffix"],
            "hybrid_config": hybrid_meta, "strategy_metadata": strategy_metadata,
            "beat_analysis": {"bpm": beat_result.tempo, "bar_duration_s": beat_result.bar_duration, "num_bars": len(beat_result.bar_times)},
            "beat_times": [float(t) for t in beat_result.beat_times], "bar_times": [float(t) for t in beat_result.bar_times],
            "bar_energies": list(beat_result.bar_energies), "bar_spectral_centroids": list(beat_result.bar_spectral_centroids),
            "bar_spectral_bandwidths": list(beat_result.bar_spectral_bandwidths), "quiet_gate": gate,
            "segment_layout_applied": False, "suppressed_cut_points_sec": [float(c.t) for c in self._last_suppressed_cut_points],
            "guard_adjustments": kept, "guard_shift_stats": stats,
            "precision_guard_ok": bool(stats["avg_shift_ms"] <= PRECISION_GUARD_AVG_MS and stats["p95_shift_ms"] <= PRECISION_GUARD_P95_MS),
            "precision_guard_threshold_ms": {"avg": PRECISION_GUARD_AVG_MS, "p95": PRECISION_GUARD_P95_MS},
            "timings": {"separate_s": t_sep, "detect_s": max(0.0, t_base - t_sep) + t_det, "finalize_s": t_fin}}
        if stereo:
            result.update({"vocal_track_stereo": base.get("vocal_track_stereo"),
                           "instrumental_track_stereo": base.get("instrumental_track_stereo"), "mono_mix": mono})
        return result

    # ------------------------------------------------------------------------------------------
    def _single_segment_fields(self, vocal_track: np.ndarray, n_samples: int, vocal_dev=None) -> Dict:
        """`_create_single_segment_result` (`:2682-2747`): one segment labelled by `_estimate_vocal_presence` (`:2404-2410`)."""
        self._last_guard_adjustments_raw = []
        self._last_suppressed_cut_points = []
        flags = self._classify_segments_vocal_presence(vocal_track, [0, len(vocal_track)], vocal_dev=vocal_dev) \
            if (vocal_track is not None and getattr(vocal_track, "size", 0)) else []
        has_vocal = bool(flags[0]) if flags else False
        sr = float(self.sample_rate)
        return {"cuts_samples": [0, int(n_samples)], "cuts_sec": [0.0, n_samples / sr], "segment_vocal_flags": [has_vocal],
                "segment_spans": [(0, int(n_samples))], "segment_durations": [n_samples / sr], "segment_layout_applied": False,
                "suppressed_cut_points_sec": [], "single_segment": True}

    # ---- post-path boundary policy (reference `seamless_splitter.py:521-669`) -----------
    def _vocal_on_device(self, vocal_audio: np.ndarray, vocal_dev=None):
        return vocal_dev if vocal_dev is not None else self._context().to_device(np.ascontiguousarray(vocal_audio, dtype=np.float32))

    def _classify_segments_vocal_presence(self, vocal_audio: np.ndarray, cut_points: Sequence[int], marker_segments=None,
                                          pure_music_segments=None, instrumental_audio=None, original_audio=None, *,
                                          vocal_dev=None) -> List[bool]:
        """`:2276-2403`: a segment is `human` when at least `segment_vocal_activity_ratio` of its 50 ms / 20 ms RMS frames
        exceed `segment_vocal_threshold_db`.  All segments' frames come from ONE `ac_segment_frame_rms` launch."""
        n_seg = max(len(cut_points) - 1, 0)
        self._last_segment_classification_debug = []
        if n_seg == 0:
            return []
        sr = self.sample_rate
        if sr <= 0 or vocal_audio is None or getattr(vocal_audio, "size", 0) == 0:
            self._last_segment_classification_debug = [{"index": i, "reason": "fallback_invalid_input", "decision": True} for i in range(n_seg)]
            return [True] * n_seg
        ratio_thr = float(get_config("quality_control.segment_vocal_activity_ratio", 0.10))
        thr_db = float(get_config("quality_control.segment_vocal_threshold_db", -50.0))
        hop = max(1, int(0.02 * sr))
        frame_length = max(hop * 2, int(0.05 * sr))
        n = len(vocal_audio)
        a = np.clip(np.asarray(cut_points[:-1], dtype=np.int64), 0, n)
        b = np.maximum(a, np.clip(np.asarray(cut_points[1:], dtype=np.int64), 0, n))
        hip = self._context()
        # segments already measured in this policy pass (the three classification rounds of `_apply_boundary_policy` mostly
        # see the same segments) come from the cache; the rest go to the GPU in two launches
        cache = getattr(self, "_segment_measure_cache", None)
        key = [(int(a[i]), int(b[i])) for i in range(n_seg)]
        need = [i for i in range(n_seg) if b[i] > a[i] and (cache is None or key[i] not in cache)]
        measured = {}
        if need:
            dev = self._vocal_on_device(vocal_audio, vocal_dev)
            nd = np.asarray(need, dtype=np.int64)
            ss = hip.segment_sumsq_peak(dev, a[nd], b[nd])[0]
            long_ix = nd[(b[nd] - a[nd]) >= frame_length]
            fr = dict(zip(long_ix.tolist(), hip.segment_frame_rms(dev, a[long_ix], b[long_ix], frame_length, hop))) if long_ix.size else {}
            for j, i in enumerate(need):
                measured[key[i]] = (float(ss[j]), fr.get(i))
            if cache is not None:
                cache.update(measured)
        look = (lambda k: cache.get(k)) if cache is not None else (lambda k: measured.get(k))
        frames = {i: look(key[i])[1] for i in range(n_seg) if b[i] > a[i] and look(key[i])[1] is not None}
        sumsq = {i: look(key[i])[0] for i in range(n_seg) if b[i] > a[i]}
        flags: List[bool] = []
        debug: List[Dict] = []
        for i in range(n_seg):
            t0, t1 = int(a[i]) / sr, int(b[i]) / sr
            dur = max(t1 - t0, 1e-6)
            size = int(b[i] - a[i])
            ratio = seconds = 0.0
            rms_db = None
            if i in sumsq:          # np.sqrt(np.mean(np.square(seg)) + 1e-12) of the float32 segment
                rms_db = 20.0 * np.log10(float(np.sqrt(np.float32(sumsq[i] / size) + np.float32(1e-12))))
            if i in frames:
                active = (20.0 * np.log10(frames[i] + 1e-12)) > thr_db
                if active.size > 0:
                    ratio = float(np.mean(active))
                    seconds = float(min(dur, float(active.sum()) * (hop / sr)))
            elif size > 0 and rms_db > thr_db:
                ratio, seconds = 1.0, dur
            decision = ratio >= ratio_thr
            why = "vocal_activity_ratio_gte_threshold" if decision else "vocal_activity_ratio_lt_threshold"
            debug.append({"index": i, "start_s": t0, "end_s": t1, "duration_s": dur, "vocal_activity_ratio": ratio,
                          "vocal_activity_seconds": seconds, "activity_ratio_threshold": ratio_thr, "activity_threshold_db": thr_db,
                          "rms_db": rms_db, "decision": decision, "decision_reason": why, "reason": why,
                          "decision_threshold_db": thr_db, "threshold_source": "vocal_activity_ratio"})
            flags.append(bool(decision))
        self._last_segment_classification_debug = debug
        return flags

    def _refine_boundaries_local_valley(self, sample_boundaries: List[int], vocal_audio: np.ndarray, cfg: Dict, *, min_gap_s: float,
                                        protected_intervals_s=None, vocal_dev=None) -> List[int]:
        """`:2613-2680`: every interior boundary may move to the quietest 5 ms of its +-radius neighbourhood when that is at
        least `min_drop_db` quieter; all neighbourhoods are searched in ONE `ac_local_valley` launch on the boundaries as
        they stand, then the moves are accepted left to right (a move only tightens its neighbours' gap checks, which use
        the already-updated left boundary exactly as the reference's in-place loop does)."""
        if vocal_audio is None or vocal_audio.size == 0 or len(sample_boundaries) <= 2:
            return sample_boundaries
        sr = float(self.sample_rate)
        radius = max(1, int(float(cfg.get("search_radius_ms", 200)) / 1000.0 * sr))
        win = max(1, int(float(cfg.get("window_ms", 20)) / 1000.0 * sr))
        drop_db = float(cfg.get("min_drop_db", 3.0))
        micro = float(get_config("segment_layout.micro_merge_s", 0.0) or 0.0)
        piece = float(get_config("quality_control.segment_min_mix_piece", 0.0) or 0.0)
        min_seg = max(1, int(max(float(min_gap_s), micro, piece) * sr))
        protected = sorted((float(x), float(y)) for x, y in (protected_intervals_s or []) if float(y) > float(x))
        refined = list(sample_boundaries)
        centers = np.asarray(refined[1:-1], dtype=np.int64)
        dev = self._vocal_on_device(vocal_audio, vocal_dev)
        orig_db, min_db, min_idx = self._context().local_valley(dev, centers, radius, win)
        for k, idx in enumerate(range(1, len(refined) - 1)):
            if min_idx[k] < 0 or (orig_db[k] - min_db[k]) < drop_db:
                continue
            center = refined[idx]
            cand = max(0, center - radius) + int(min_idx[k]) + win // 2
            if any(x < cand / sr < y for x, y in protected):
                continue
            if cand <= refined[idx - 1] + min_seg or cand >= refined[idx + 1] - min_seg:
                continue
            refined[idx] = cand
        return refined

    def _merge_short_weak_human_tails_into_following_music(self, cut_points: List[int], segment_vocal_flags: List[bool],
                                                           debug_entries: List[Dict], vocal_audio: np.ndarray, *,
                                                           min_duration_s: float, layout_applied: bool, vocal_dev=None):
        """`:2145-2275`: a human segment shorter than `soft_min_s` whose RMS and peak are under 12 % / 18 % of the median
        long human segment, followed by music, becomes part of that music.  Segment energies come from one
        `ac_segment_sumsq_peak` launch; a merged pair's statistics are the sums / max of its parts."""
        debug = [dict(e) for e in (debug_entries or [])]
        if (not layout_applied or min_duration_s <= 0.0 or len(cut_points) < 3 or len(segment_vocal_flags) != len(cut_points) - 1
                or vocal_audio is None or getattr(vocal_audio, "size", 0) == 0 or self.sample_rate <= 0):
            return list(cut_points), list(segment_vocal_flags), debug
        sr = float(self.sample_rate)
        n = len(vocal_audio)
        pts = [int(p) for p in cut_points]
        flags = [bool(f) for f in segment_vocal_flags]
        while len(debug) < len(flags):
            debug.append({})
        a = np.clip(np.asarray(pts[:-1], dtype=np.int64), 0, n)
        b = np.maximum(a, np.clip(np.asarray(pts[1:], dtype=np.int64), 0, n))
        live = np.flatnonzero(b > a)
        ss = np.zeros(len(a)); pk = np.zeros(len(a))
        if live.size:
            s_live, p_live = self._context().segment_sumsq_peak(self._vocal_on_device(vocal_audio, vocal_dev), a[live], b[live])
            ss[live] = s_live; pk[live] = p_live
        size = (b - a).astype(np.float64)
        seg = [{"ss": float(ss[i]), "pk": float(pk[i]), "n": float(size[i])} for i in range(len(a))]

        def stat(i):
            cnt = seg[i]["n"]
            rms = float(np.sqrt(seg[i]["ss"] / cnt + 1e-12)) if cnt > 0 else 0.0
            return max(0.0, (pts[i + 1] - pts[i]) / sr), rms, (seg[i]["pk"] if cnt > 0 else 0.0)

        st = [stat(i) for i in range(len(flags))]
        ref_r = [r for (d, r, p), f in zip(st, flags) if f and d >= min_duration_s and r > 0.0]
        ref_p = [p for (d, r, p), f in zip(st, flags) if f and d >= min_duration_s and p > 0.0]
        if not ref_r or not ref_p:
            return pts, flags, debug[:len(flags)]
        rr = float(np.median(np.asarray(ref_r, dtype=np.float64)))
        rp = float(np.median(np.asarray(ref_p, dtype=np.float64)))
        w_r = float(get_config("quality_control.short_human_tail_rms_ratio", 0.12) or 0.12)
        w_p = float(get_config("quality_control.short_human_tail_peak_ratio", 0.18) or 0.18)
        why = "merged_short_weak_human_tail_into_following_music"
        i = 0
        while i < len(flags) - 1:
            d, r, p = stat(i)
            if not (flags[i] and not flags[i + 1] and d < min_duration_s and r <= rr * w_r and p <= rp * w_p):
                i += 1
                continue
            t0, t1 = pts[i] / sr, pts[i + 2] / sr
            pts.pop(i + 1)
            seg[i:i + 2] = [{"ss": seg[i]["ss"] + seg[i + 1]["ss"], "pk": max(seg[i]["pk"], seg[i + 1]["pk"]), "n": seg[i]["n"] + seg[i + 1]["n"]}]
            left, right = debug[i], debug[i + 1]
            merged = dict(right or left or {})
            span = max(t1 - t0, 1e-6)
            voiced = min(span, float((left or {}).get("vocal_activity_seconds", 0.0) or 0.0) + float((right or {}).get("vocal_activity_seconds", 0.0) or 0.0))
            origin = []
            for e in (left, right):
                if e:
                    origin.extend(e.get("merged_from_segments", [e.get("index")]))
            merged.update({"index": i, "start_s": t0, "end_s": t1, "duration_s": span, "vocal_activity_seconds": voiced,
                           "vocal_activity_ratio": voiced / span, "decision": False, "decision_reason": why, "reason": why,
                           "merged_from_segments": sorted({int(x) for x in origin if x is not None})})
            flags[i:i + 2] = [False]
            debug[i:i + 2] = [merged]
        for k, e in enumerate(debug[:len(flags)]):
            e["index"] = k
        return pts, flags, debug[:len(flags)]

    def _split_at_sample_level(self, audio: np.ndarray, final_cut_points: List[int], *, segment_flags: Optional[List[bool]] = None,
                               debug_entries: Optional[List[Dict]] = None):
        """`:2006-2144`: slices between consecutive cut points; a slice shorter than 10 ms is glued to the next one (a
        trailing one to the previous).  Slices are views of `audio` unless a merge forces a copy."""
        spans, flags = self._sample_level_spans(len(audio), final_cut_points, segment_flags)
        return [audio[lo:hi] for lo, hi in spans], flags, None

    def _sample_level_spans(self, n: int, final_cut_points: List[int], segment_flags: Optional[List[bool]] = None):
        """The spans `_split_at_sample_level` slices a track of `n` samples into, and their merged flags (None without
        `segment_flags`); kept in `_last_segment_spans` too."""
        keep = max(1, int(0.01 * self.sample_rate))
        spans: List[List[int]] = []
        flags: Optional[List[bool]] = [] if segment_flags is not None else None
        pending: Optional[List[int]] = None
        pending_flag: Optional[bool] = None
        for i in range(len(final_cut_points) - 1):
            lo = max(0, min(int(final_cut_points[i]), n)); hi = max(lo, min(int(final_cut_points[i + 1]), n))
            span = [lo, hi] if hi > lo else None
            flag = bool(segment_flags[i]) if (segment_flags is not None and i < len(segment_flags)) else True
            if pending is not None:
                span = [pending[0], span[1]] if span is not None else list(pending)
                flag = bool(pending_flag) or flag
                pending, pending_flag = None, None
            if int(final_cut_points[i + 1]) - int(final_cut_points[i]) >= keep and span is not None:
                spans.append(span)
                if flags is not None:
                    flags.append(flag)
            elif span is not None:
                pending, pending_flag = span, flag
        if pending is not None:
            if spans:
                spans[-1][1] = pending[1]
                if flags is not None:
                    flags[-1] = bool(flags[-1]) or bool(pending_flag)
            else:
                spans.append(pending)
                if flags is not None:
                    flags.append(bool(pending_flag))
        self._last_segment_spans = [tuple(sp) for sp in spans]
        return self._last_segment_spans, flags

    def _apply_boundary_policy(self, bounds: List[int], vocal_track: np.ndarray, n_samples: int,
                               cache: Optional[TrackFeatureCache], *, vocal_dev=None, lyrics_alignment: Optional[Dict] = None) -> Dict:
        """`:521-669`: classify -> layout refiner -> classify -> local valley -> classify -> weak-tail merge -> sample-level
        split.  Returns the manifest-facing fields.  `lyrics_alignment` (mode `vpbd_asr` only): the layout refiner then reads the
        vocal stem's RMS, the timeline's sentence / region boundaries and word intervals, and the local valley search keeps out of
        the words (`:547-551,575-584,624-628`)."""
        from ..cutting.segment_layout_refiner import Segment as LayoutSegment, derive_layout_config, refine_layout
        sr = self.sample_rate
        cuts = sorted(set(int(c) for c in bounds))
        self._segment_measure_cache = {}
        try:
            return self._boundary_policy_steps(cuts, vocal_track, n_samples, cache, vocal_dev, lyrics_alignment)
        finally:
            self._segment_measure_cache = None

    def _boundary_policy_steps(self, cuts: List[int], vocal_track: np.ndarray, n_samples: int, cache, vocal_dev,
                               lyrics_alignment: Optional[Dict] = None) -> Dict:
        from ..cutting.segment_layout_refiner import Segment as LayoutSegment, derive_layout_config, refine_layout
        sr = self.sample_rate
        flags = self._classify_segments_vocal_presence(vocal_track, cuts, vocal_dev=vocal_dev)
        raw = dict(get_config("segment_layout", {}) or {})
        micro = get_config("quality_control.segment_min_mix_piece", None)
        if micro is not None:
            raw.setdefault("micro_merge_s", float(micro)); raw.setdefault("enable", bool(float(micro) > 0.0))
        smax = get_config("quality_control.segment_max_duration", None)
        if smax is not None:
            raw.setdefault("soft_max_s", float(smax))
        raw.setdefault("min_gap_s", float(get_config("quality_control.min_split_gap", 1.0)))
        raw.setdefault("beat_snap_ms", float(get_config("segment_layout.beat_snap_ms", 0.0) or 0.0))
        asr = lyrics_alignment is not None
        if asr:
            cache = self._build_vocal_layout_feature_cache(cache, vocal_track, vocal_dev=vocal_dev)
        lcfg = derive_layout_config(raw, cache, sample_rate=sr)
        applied = False
        if lcfg.enable and len(cuts) >= 2:
            edges = [c / float(sr) for c in cuts]
            res = refine_layout([LayoutSegment(edges[i], edges[i + 1], "human" if flags[i] else "music") for i in range(len(edges) - 1)],
                                self._last_guard_adjustments_raw, config=lcfg, sample_rate=sr,
                                suppressed_cut_points=self._last_suppressed_cut_points, features=cache,
                                asr_boundary_times=self._collect_lyrics_boundary_times(lyrics_alignment) if asr else None,
                                asr_word_intervals=self._collect_lyrics_word_intervals(lyrics_alignment) if asr else None)
            if res.segments:
                times = [res.segments[0].start] + [sg.end for sg in res.segments]
                upd = [max(0, min(int(round(t * sr)), n_samples)) for t in times]
                if upd:
                    upd[0] = 0; upd[-1] = n_samples
                upd = sorted(set(upd))
                if upd != cuts:
                    applied = True
                cuts = upd if upd else cuts
                self._last_guard_adjustments_raw = list(res.adjustments)
                self._last_suppressed_cut_points = list(res.suppressed_points or [])
                flags = self._classify_segments_vocal_presence(vocal_track, cuts, vocal_dev=vocal_dev)
        local = get_config("quality_control.local_boundary_refine", {}) or {}
        if local.get("enable") and len(cuts) >= 2:
            ref = self._refine_boundaries_local_valley(cuts, vocal_track, local, min_gap_s=float(get_config("quality_control.min_split_gap", 1.0)),
                                                       protected_intervals_s=self._collect_lyrics_word_intervals(lyrics_alignment) if asr else None,
                                                       vocal_dev=vocal_dev)
            if list(ref) != cuts:
                cuts = list(ref); applied = True
                flags = self._classify_segments_vocal_presence(vocal_track, cuts, vocal_dev=vocal_dev)
        c2, f2, dbg = self._merge_short_weak_human_tails_into_following_music(
            cuts, flags, list(getattr(self, "_last_segment_classification_debug", [])), vocal_track,
            min_duration_s=float(getattr(lcfg, "soft_min_s", 0.0) or 0.0), layout_applied=applied, vocal_dev=vocal_dev)
        if list(c2) != cuts:
            cuts, flags, applied = list(c2), list(f2), True
            self._last_segment_classification_debug = dbg
        _, merged_flags, _ = self._split_at_sample_level(np.empty(n_samples, dtype=np.int8), cuts, segment_flags=flags)
        spans = list(self._last_segment_spans)
        return {"cuts_samples": list(cuts), "cuts_sec": [c / float(sr) for c in cuts], "segment_vocal_flags": list(merged_flags or []),
                "segment_spans": spans, "segment_durations": [(hi - lo) / float(sr) for lo, hi in spans],
                "segment_layout_applied": bool(applied),
                "suppressed_cut_points_sec": [float(c.t) for c in self._last_suppressed_cut_points]}

    # ---- mode `vpbd_asr`: what the timeline feeds into the boundary policy (reference `:896-938,1880-2004`) ----------------
    def _build_vocal_layout_feature_cache(self, cache: Optional[TrackFeatureCache], vocal_track: Optional[np.ndarray], *, vocal_dev=None):
        """A copy of the cache whose RMS series follows the VOCAL stem (the layout refiner's valley rescue then looks for quiet
        singing, not a quiet mix): `librosa.feature.rms` of the stem at `max(2 hop, 0.1 s)` per frame and the cache's hop, padded with
        its last value or cropped to the cache's frame count.  One `ac_frame_rms` launch on the resident stem."""
        if cache is None or vocal_track is None:
            return cache
        sr, hop = int(getattr(cache, "sr", 0) or 0), int(getattr(cache, "hop_length", 0) or 0)
        if sr <= 0 or hop <= 0 or np.size(vocal_track) == 0:
            return cache
        frame = max(2 * hop, int(round(sr * 0.1)))
        try:            # as in the reference (`:936-938`): a stem shorter than one frame or a frame beyond the kernel's limit keeps the mix cache
            rms = self._context().frame_rms(self._vocal_on_device(vocal_track, vocal_dev), frame, hop).cpu().numpy().astype(np.float32, copy=False)
        except Exception as exc:
            logger.debug("[Layout] vocal RMS feature cache not built: %s", exc)
            return cache
        if rms.size == 0:
            return cache
        want = int(cache.frame_count())
        if want > 0 and rms.size != want:
            rms = np.pad(rms, (0, want - rms.size), constant_values=float(rms[-1])) if rms.size < want else rms[:want]
        return dataclasses.replace(cache, rms_series=rms, rms_max=float(np.max(rms)))

    def _restore_guard_points_outside_lyrics_words(self, final_cut_points: List[int], adjustments: Sequence, word_intervals, *,
                                                   sample_count: int, min_gap_s: float):
        """-> (boundaries, adjustments or None when nothing changed).  A guard may push a cut that lay between two words into
        one; such a cut goes back to its raw time when that keeps `min_gap_s` to both neighbours and is not an end of the track.
        The restored cut's adjustment is rewritten as "not moved"."""
        if not final_cut_points or not adjustments or not word_intervals:
            return list(final_cut_points), None
        sr = float(self.sample_rate)
        min_gap = max(0, int(round(float(min_gap_s) * sr)))
        words = sorted(word_intervals)

        def inside(t: float) -> bool:
            for a, b in words:
                if a < t < b:
                    return True
                if a >= t:
                    break
            return False

        to_sample = lambda t: max(0, min(int(round(t * sr)), sample_count))
        points = sorted({max(0, min(int(p), sample_count)) for p in final_cut_points})
        restored = set()
        for adj in adjustments:
            raw_t, final_t = float(adj.raw_time), float(adj.final_time)
            if not inside(final_t) or inside(raw_t):
                continue
            raw, final = to_sample(raw_t), to_sample(final_t)
            if final not in points or raw in (0, sample_count):
                continue
            trial = sorted(raw if p == final else p for p in points)
            i = trial.index(raw)
            if (i > 0 and trial[i] - trial[i - 1] < min_gap) or (i < len(trial) - 1 and trial[i + 1] - trial[i] < min_gap):
                continue
            points = trial
            restored.add(raw_t)
        if not restored:
            return list(final_cut_points), None
        from ..cutting.refine import CutAdjustment
        return points, [CutAdjustment(raw_time=a.raw_time, guard_time=a.raw_time, final_time=a.raw_time, score=a.score,
                                      guard_shift_ms=0.0, final_shift_ms=0.0) if float(a.raw_time) in restored else a
                        for a in adjustments]

    @staticmethod
    def _timeline_rows(lyrics_alignment, key: str):
        timeline = lyrics_alignment.get("timeline") if isinstance(lyrics_alignment, dict) else None
        rows = (timeline.get(key, []) or []) if isinstance(timeline, dict) else []
        return [r for r in rows if isinstance(r, dict)]

    @staticmethod
    def _collect_lyrics_word_intervals(lyrics_alignment: Optional[Dict]) -> List[Tuple[float, float]]:
        """(start, end) of every well-formed word of `lyrics_alignment["timeline"]`, sorted, duplicates dropped."""
        out = set()
        for w in SeamlessSplitter._timeline_rows(lyrics_alignment, "words"):
            try:
                a, b = float(w.get("start_s")), float(w.get("end_s"))
            except (TypeError, ValueError):
                continue
            if b > a:
                out.add((a, b))
        return sorted(out)

    @staticmethod
    def _collect_lyrics_boundary_times(lyrics_alignment: Optional[Dict]) -> List[float]:
        """every sentence end and every edge of a VAD region, > 0, sorted, duplicates dropped: soft priors of the layout refiner."""
        values = [s.get("end_s") for s in SeamlessSplitter._timeline_rows(lyrics_alignment, "sentences")]
        for r in SeamlessSplitter._timeline_rows(lyrics_alignment, "vad_regions"):
            values += [r.get("start_s"), r.get("end_s")]
        out = set()
        for v in values:
            try:
                v = float(v)
            except (TypeError, ValueError):
                continue
            if v > 0.0:
                out.add(v)
        return sorted(out)

    def _rms2048_db(self, wave: np.ndarray, dev=None) -> np.ndarray:
        hip = self._context()
        x = dev if dev is not None else hip.to_device(np.ascontiguousarray(wave, dtype=np.float32))
        hop = max(1, int(0.01 * self.sample_rate))
        rms = hip.frame_rms(x, 2048, hop).cpu().numpy()
        return rms, 20.0 * np.log10(rms + 1e-12)

    def _find_no_vocal_runs(self, vocal_audio: np.ndarray, min_duration: float, *, vocal_dev=None):
        """`seamless_splitter.py:1706-1790`."""
        sr = self.sample_rate
        hop = max(1, int(0.01 * sr))
        rms, db = self._rms2048_db(vocal_audio, vocal_dev)
        noise_pct = float(get_config("quality_control.enforce_quiet_cut.floor_percentile", 10))
        voice_pct = float(get_config("pure_vocal_detection.pause_stats_adaptation.voice_percentile_hint", 90))
        noise_db = float(np.percentile(db, np.clip(noise_pct, 0, 50)))
        voice_db = float(np.percentile(db, np.clip(voice_pct, 50, 100)))
        delta_db = float(get_config("pure_vocal_detection.pause_stats_adaptation.delta_db", 3.0))
        thr_db = max(noise_db + delta_db, 0.5 * (noise_db + voice_db))
        active = db > thr_db
        frame_sec = hop / float(sr)
        close_k = max(1, int(int(get_config("pure_vocal_detection.pause_stats_adaptation.morph_close_ms", 150)) / 1000.0 / frame_sec))
        open_k = max(1, int(int(get_config("pure_vocal_detection.pause_stats_adaptation.morph_open_ms", 50)) / 1000.0 / frame_sec))
        inactive = ~_remove_true_runs(_fill_false_runs(active, close_k), open_k)
        times = (np.arange(len(rms)) * hop).astype(int) / float(sr)
        n = len(vocal_audio) if vocal_audio is not None else int(vocal_dev.numel())
        spans = []
        for a, b, v in _bool_runs(inactive):
            if not v:
                continue
            st = float(times[a])
            en = float(times[b]) if b < len(inactive) else float(n / float(sr))
            if en - st >= float(min_duration):
                spans.append((st, en))
        return spans

    def _finalize_and_filter_cuts_v2(self, cut_candidates, audio_for_split: np.ndarray,
                                     pure_vocal_audio: Optional[np.ndarray] = None, *, mix_dev=None, vocal_dev=None) -> CutRefineResult:
        """`seamless_splitter.py:1792-1879` (quirk Q1: floor_percentile 0.5 is read as a fraction)."""
        sr = self.sample_rate
        if sr <= 0 or audio_for_split.size == 0:
            return CutRefineResult([], [0, len(audio_for_split)], [])
        points: List[CutPoint] = []
        if isinstance(cut_candidates, list) and cut_candidates:
            first = cut_candidates[0]
            if isinstance(first, tuple) and len(first) >= 2:
                points = [CutPoint(t=float(c[0]), score=float(c[1])) for c in cut_candidates]
            elif isinstance(first, int):
                points = [CutPoint(t=float(s) / float(sr), score=1.0) for s in cut_candidates]
            else:
                points = [CutPoint(t=float(t), score=1.0) for t in cut_candidates]
        if not points:
            return CutRefineResult([], [0, len(audio_for_split)], [])
        min_gap_s = float(get_config("quality_control.min_split_gap", 1.0))
        try:
            max_keep = int(get_config("pure_vocal_detection.valley_scoring.max_kept_after_nms", 150))
        except Exception:
            max_keep = None
        guard_enabled = bool(get_config("quality_control.enforce_quiet_cut.enable", False))
        guard_db = float(get_config("quality_control.enforce_quiet_cut.guard_db", 2.5))
        search_right_ms = float(get_config("quality_control.enforce_quiet_cut.search_right_ms", 150))
        guard_win_ms = float(get_config("quality_control.enforce_quiet_cut.win_ms", 80))
        floor_db = -60.0
        if guard_enabled:
            from ..analysis.prefetch import guard_floor_db
            if get_config("quality_control.enforce_quiet_cut.floor_db_override", None) is not None:
                floor_db = guard_floor_db(np.zeros(0))
            else:
                mono = audio_for_split if audio_for_split.ndim == 1 else np.mean(audio_for_split, axis=0)
                if mono.size > 0:
                    _, rms_db = self._rms2048_db(mono, mix_dev if audio_for_split.ndim == 1 else None)
                    floor_db = guard_floor_db(rms_db)
        ctx = CutContext(sr=sr, mix_wave=audio_for_split, vocal_wave=pure_vocal_audio, mix_dev=mix_dev, vocal_dev=vocal_dev,
                         hip=self._context())
        use_vocal_guard = pure_vocal_audio is not None
        topk_cfg = get_config("quality_control.nms_topk_per_10s", None)
        result = finalize_cut_points(
            ctx, points, use_vocal_guard_first=use_vocal_guard, min_gap_s=min_gap_s, max_keep=max_keep,
            topk_per_10s=int(topk_cfg) if topk_cfg is not None else None,
            nms_window_s=float(get_config("quality_control.nms_window_s", 10.0)), guard_db=guard_db,
            search_right_ms=search_right_ms, guard_win_ms=guard_win_ms, floor_db=floor_db,
            enable_mix_guard=guard_enabled, enable_vocal_guard=(guard_enabled and use_vocal_guard))
        self._last_guard_adjustments_raw = list(result.adjustments or [])
        bounds = sorted(set(result.sample_boundaries or [0, len(audio_for_split)]))
        return CutRefineResult(result.final_points, bounds, list(result.adjustments or []), result.suppressed_points)


__all__ = ["SeamlessSplitter"]
