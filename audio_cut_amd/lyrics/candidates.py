"""Boundary candidates a lyrics timeline offers the VPBD pool (reference `src/audio_cut/lyrics/candidates.py`): the middle of
every word gap of at least `min_word_gap_s`, every sentence end (a little more for terminal punctuation, Latin or CJK), and both
edges of every region of the provider's music VAD.  Soft priors: the scorer and the planner decide."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

from ..cutting.cut_candidate import CandidateSource, CutCandidate
from .models import LyricsTimeline

_SENTENCE_ENDINGS = (".", "!", "?", "。", "！", "？")


@dataclass
class LyricsBoundaryCandidateGenerator:
    min_word_gap_s: float = 0.35
    max_word_gap_s: float = 1.5
    sentence_end_score: float = 0.75
    mvad_boundary_score: float = 0.45

    def generate(self, timeline: LyricsTimeline) -> List[CutCandidate]:
        out = self._word_gaps(timeline.words) + self._sentence_ends(timeline.sentences) + self._mvad_edges(timeline.vad_regions)
        return sorted(out, key=lambda c: (c.t, c.source.value))

    def _word_gaps(self, words) -> List[CutCandidate]:
        out = []
        full = max(self.max_word_gap_s, self.min_word_gap_s)
        for a, b in zip(words, words[1:]):
            gap = b.start_s - a.end_s
            if gap < self.min_word_gap_s:
                continue
            out.append(CutCandidate(t=(a.end_s + b.start_s) / 2.0, score=min(1.0, gap / full), source=CandidateSource.LYRICS_GAP,
                                    reasons=["word_gap"], meta={"gap_s": gap, "left_word": a.text, "right_word": b.text}))
        return out

    def _sentence_ends(self, sentences) -> List[CutCandidate]:
        out = []
        for s in sentences:
            reasons, score = ["sentence_end"], self.sentence_end_score
            if s.text.strip().endswith(_SENTENCE_ENDINGS):
                reasons.append("punctuation_end")
                score = min(1.0, score + 0.1)
            if s.confidence is not None:
                score *= s.confidence
            out.append(CutCandidate(t=s.end_s, score=score, source=CandidateSource.SENTENCE_END, reasons=reasons, meta={"text": s.text}))
        return out

    def _mvad_edges(self, regions) -> List[CutCandidate]:
        out = []
        for r in regions:
            score = self.mvad_boundary_score if r.confidence is None else self.mvad_boundary_score * r.confidence
            out.append(CutCandidate(t=r.start_s, score=score, source=CandidateSource.MVAD_BOUNDARY, reasons=["mvad_start"], meta={"kind": r.kind}))
            out.append(CutCandidate(t=r.end_s, score=score, source=CandidateSource.MVAD_BOUNDARY, reasons=["mvad_end"], meta={"kind": r.kind}))
        return out


__all__ = ["LyricsBoundaryCandidateGenerator"]
