"""Lyrics of every exported segment (reference `src/audio_cut/lyrics/segment_attach.py`): a word belongs to a segment when at
least `min_word_overlap_ratio` of its own length lies inside it.  Words are joined with a space, or with nothing when every one
of them holds a CJK ideograph."""
from __future__ import annotations

import re
from copy import deepcopy
from typing import Any, Dict, List, Mapping, Optional, Sequence

from .models import LyricsTimeline, Word

_CJK = re.compile("[\\u3400-\\u9fff\\uf900-\\ufaff]")      # CJK unified ideographs (with extension A) and compatibility ideographs


def _number(value: Any) -> Optional[float]:
    try:
        return None if value is None else float(value)
    except (TypeError, ValueError):
        return None


def _share_inside(word: Word, start: float, end: float) -> float:
    overlap = min(word.end_s, end) - max(word.start_s, start)
    return 0.0 if overlap <= 0.0 else overlap / max(word.end_s - word.start_s, 1e-9)


def _segment_lyrics(words: Sequence[Word]) -> Dict[str, Any]:
    words = sorted(words, key=lambda w: (w.start_s, w.end_s))
    texts = [w.text for w in words]
    joiner = "" if all(_CJK.search(t) for t in texts) else " "
    return {"text": joiner.join(texts), "words": [w.to_dict() for w in words], "start": words[0].start_s, "end": words[-1].end_s}


def attach_lyrics_to_segments(segments: Sequence[Mapping[str, Any]], timeline: LyricsTimeline, *,
                              min_word_overlap_ratio: float = 0.5) -> List[Dict[str, Any]]:
    """Copies of `segments` (rows with `start` / `end` seconds), each with a `lyrics` object or None."""
    out: List[Dict[str, Any]] = []
    for seg in segments:
        row = deepcopy(dict(seg))
        start, end = _number(row.get("start")), _number(row.get("end"))
        row["lyrics"] = None
        if start is not None and end is not None and end > start:
            inside = [w for w in timeline.words if _share_inside(w, start, end) >= min_word_overlap_ratio]
            if inside:
                row["lyrics"] = _segment_lyrics(inside)
        out.append(row)
    return out


__all__ = ["attach_lyrics_to_segments"]
