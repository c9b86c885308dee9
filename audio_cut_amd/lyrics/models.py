"""Words, sentences, singing regions and the full-track timeline a lyrics provider returns (reference
`src/audio_cut/lyrics/models.py`).  All times are seconds on the track's own axis.  Every item checks itself when it is built;
a timeline loaded with `from_dict(strict=False)` drops the items that fail and lists them in `warnings`, and an end that
overshoots the track by at most a millisecond (an ASR engine's rounding) is clamped to the duration instead of dropped."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, Iterable, List, Optional

from ..exceptions import TimelineValidationError

_EPS = 1e-9
_OVERSHOOT_S = 0.001


def _opt_float(value: Any, name: str) -> Optional[float]:
    if value is None:
        return None
    try:
        return float(value)
    except (TypeError, ValueError) as exc:
        raise TimelineValidationError(f"{name} must be a number or null") from exc


def _req_float(value: Any, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError) as exc:
        raise TimelineValidationError(f"{name} must be a number") from exc


@dataclass
class _Timed:
    start_s: float
    end_s: float
    confidence: Optional[float] = None

    def validate(self, duration_s: Optional[float] = None) -> None:
        if self.start_s < 0.0:
            raise TimelineValidationError("start_s must be >= 0")
        if self.end_s <= self.start_s + _EPS:
            raise TimelineValidationError("end_s must be greater than start_s")
        if duration_s is not None and self.end_s > duration_s + _EPS:
            raise TimelineValidationError("end_s exceeds timeline duration")
        if self.confidence is not None and (self.confidence < 0.0 or self.confidence > 1.0):
            raise TimelineValidationError("confidence must be in [0, 1]")

    def _set_span(self, start_s: Any, end_s: Any, confidence: Any) -> None:
        self.start_s, self.end_s = float(start_s), float(end_s)
        self.confidence = _opt_float(confidence, "confidence")
        self.validate()


class _Texted(_Timed):
    """Word and Sentence: a span with a non-empty text.  `_label` names the fields in messages."""
    _label = "item"

    def __init__(self, text: str, start_s: float, end_s: float, confidence: Optional[float] = None) -> None:
        self.text = str(text)
        self._set_span(start_s, end_s, confidence)
        if not self.text:
            raise TimelineValidationError(f"{self._label} text must not be empty")

    @classmethod
    def from_dict(cls, data: Dict[str, Any]):
        lab = cls._label
        return cls(text=str(data.get("text", "")), start_s=_req_float(data.get("start_s"), f"{lab}.start_s"),
                   end_s=_req_float(data.get("end_s"), f"{lab}.end_s"), confidence=_opt_float(data.get("confidence"), f"{lab}.confidence"))

    def to_dict(self) -> Dict[str, Any]:
        return {"text": self.text, "start_s": self.start_s, "end_s": self.end_s, "confidence": self.confidence}

    def __eq__(self, other: object) -> bool:
        return type(other) is type(self) and self.to_dict() == other.to_dict()      # type: ignore[attr-defined]

    def __repr__(self) -> str:
        return f"{type(self).__name__}({self.text!r}, {self.start_s}, {self.end_s}, confidence={self.confidence})"


class Word(_Texted):
    """One ASR word."""
    _label = "word"


class Sentence(_Texted):
    """One sentence-level phrase span."""
    _label = "sentence"


class VadRegion(_Timed):
    """A region the provider's music VAD reports; `kind == "singing"` ones penalise cuts inside them."""

    def __init__(self, start_s: float, end_s: float, confidence: Optional[float] = None, kind: str = "singing") -> None:
        self.kind = str(kind or "singing")
        self._set_span(start_s, end_s, confidence)

    @classmethod
    def from_dict(cls, data: Dict[str, Any]) -> "VadRegion":
        return cls(start_s=_req_float(data.get("start_s"), "vad_region.start_s"), end_s=_req_float(data.get("end_s"), "vad_region.end_s"),
                   confidence=_opt_float(data.get("confidence"), "vad_region.confidence"), kind=str(data.get("kind", "singing")))

    def to_dict(self) -> Dict[str, Any]:
        return {"start_s": self.start_s, "end_s": self.end_s, "confidence": self.confidence, "kind": self.kind}

    def __eq__(self, other: object) -> bool:
        return type(other) is VadRegion and self.to_dict() == other.to_dict()

    def __repr__(self) -> str:
        return f"VadRegion({self.start_s}, {self.end_s}, confidence={self.confidence}, kind={self.kind!r})"


def _span_key(item: _Timed):
    return (item.start_s, item.end_s)


@dataclass
class LyricsTimeline:
    """Full-track lyrics timeline: a soft prior for the boundary planner, never a hard cut list."""

    words: List[Word] = field(default_factory=list)
    sentences: List[Sentence] = field(default_factory=list)
    vad_regions: List[VadRegion] = field(default_factory=list)
    duration_s: Optional[float] = None
    source: str = "unknown"
    warnings: List[str] = field(default_factory=list)
    meta: Dict[str, Any] = field(default_factory=dict)

    def __post_init__(self) -> None:
        self.duration_s = _opt_float(self.duration_s, "duration_s")
        if self.duration_s is not None and self.duration_s <= 0.0:
            raise TimelineValidationError("duration_s must be positive")
        self.words = sorted(self.words, key=_span_key)
        self.sentences = sorted(self.sentences, key=_span_key)
        self.vad_regions = sorted(self.vad_regions, key=_span_key)
        self.validate(strict=True)

    @classmethod
    def from_dict(cls, data: Dict[str, Any], *, strict: bool = False) -> "LyricsTimeline":
        duration_s = _opt_float(data.get("duration_s"), "duration_s")
        warnings: List[str] = list(data.get("warnings", []))
        groups = [_load(kind, data.get(key, []), duration_s, strict, warnings)
                  for kind, key in ((Word, "words"), (Sentence, "sentences"), (VadRegion, "vad_regions"))]
        return cls(words=groups[0], sentences=groups[1], vad_regions=groups[2], duration_s=duration_s,
                   source=str(data.get("source", "unknown")), warnings=warnings, meta=dict(data.get("meta", {})))

    def validate(self, *, strict: bool = True) -> None:
        errors: List[str] = []
        for name, items in (("words", self.words), ("sentences", self.sentences), ("vad_regions", self.vad_regions)):
            for i, item in enumerate(items):
                try:
                    item.validate(self.duration_s)
                except TimelineValidationError as exc:
                    errors.append(f"{name}[{i}]: {exc}")
        if errors and strict:
            raise TimelineValidationError("; ".join(errors))
        self.warnings.extend(errors)

    def is_empty(self) -> bool:
        return not (self.words or self.sentences or self.vad_regions or self.meta)

    def to_dict(self) -> Dict[str, Any]:
        """The reference's payload.  A timeline with no items and no `meta` - every acoustic mode's - keeps the six keys it has
        always had in a result; `meta` joins them as soon as there is anything to describe."""
        out: Dict[str, Any] = {"duration_s": self.duration_s, "source": self.source, "words": [w.to_dict() for w in self.words],
                               "sentences": [s.to_dict() for s in self.sentences], "vad_regions": [r.to_dict() for r in self.vad_regions],
                               "warnings": list(self.warnings)}
        if not self.is_empty():
            out["meta"] = dict(self.meta)
        return out


def _load(kind, raw_items: Iterable[Dict[str, Any]], duration_s: Optional[float], strict: bool, warnings: List[str]) -> list:
    items = []
    for i, raw in enumerate(raw_items):
        try:
            item = kind.from_dict(raw)
            if duration_s is not None and duration_s + _EPS < item.end_s <= duration_s + _OVERSHOOT_S and item.start_s < duration_s:
                item.end_s = float(duration_s)
                warnings.append(f"{kind.__name__}[{i}]: end_s clamped to timeline duration after minor rounding overshoot")
            item.validate(duration_s)
            items.append(item)
        except TimelineValidationError as exc:
            message = f"{kind.__name__}[{i}]: {exc}"
            if strict:
                raise TimelineValidationError(message) from exc
            warnings.append(message)
    return items


__all__ = ["Word", "Sentence", "VadRegion", "LyricsTimeline"]
