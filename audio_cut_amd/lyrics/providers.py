"""The provider seam of mode `vpbd_asr` (reference `src/audio_cut/lyrics/providers.py`): `LyricsProvider.align(request)` returns
the `LyricsTimeline` of one track.  Built here: the null provider, the fixture-backed `fake` provider the reference's own
integration test drives the mode with, and the selection by `lyrics_alignment.provider`.  The FireRed back ends (`sidecar`,
`cli`, `auto`) are external processes and are not built: selecting one gives a null provider that says so, so a non-strict run
falls back to the acoustic pool exactly as the reference does when nothing is configured, and a strict run raises.  A host
application's own engine is a `LyricsProvider` set as `VocalPhraseBoundaryDetector.lyrics_provider`."""
from __future__ import annotations

import json
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, Optional

from ..exceptions import LyricsAlignmentUnavailable
from .models import LyricsTimeline

_FIRERED_NOT_BUILT = "FireRed {0} back end is not built in this library: set VocalPhraseBoundaryDetector.lyrics_provider"


@dataclass
class LyricsProviderRequest:
    """What a provider gets.  `vocal_path`: the 16 kHz 16-bit mono WAV of the vocal stem, or None when no export directory was
    given; `meta["pcm16"]`: the same samples as an int16 array (absent on a host-only run); `sample_rate` is that of both."""

    vocal_path: Optional[Path]
    duration_s: Optional[float] = None
    sample_rate: Optional[int] = None
    strict: bool = False
    meta: Dict[str, Any] = field(default_factory=dict)


class LyricsProvider(ABC):
    name: str = "base"

    @abstractmethod
    def align(self, request: LyricsProviderRequest) -> LyricsTimeline:
        """The full-track lyrics timeline of `request`."""


class NullLyricsProvider(LyricsProvider):
    """Alignment switched off or not available: an empty timeline carrying the reason, or the reason raised when strict."""

    name = "null"

    def __init__(self, reason: str = "lyrics alignment disabled") -> None:
        self.reason = reason

    def align(self, request: LyricsProviderRequest) -> LyricsTimeline:
        if request.strict:
            raise LyricsAlignmentUnavailable(self.reason)
        return LyricsTimeline(duration_s=request.duration_s, source=self.name, warnings=[self.reason])


class FakeLyricsProvider(LyricsProvider):
    """Reads the timeline from a JSON file (`LyricsTimeline.to_dict()`'s layout): deterministic tests and dry runs."""

    name = "fake"

    def __init__(self, fixture_path) -> None:
        self.fixture_path = Path(fixture_path)

    def align(self, request: LyricsProviderRequest) -> LyricsTimeline:
        if not self.fixture_path.exists():
            message = f"lyrics fixture not found: {self.fixture_path}"
            if request.strict:
                raise LyricsAlignmentUnavailable(message)
            return LyricsTimeline(duration_s=request.duration_s, source=self.name, warnings=[message])
        payload = json.loads(self.fixture_path.read_text(encoding="utf-8"))
        payload.setdefault("source", self.name)
        if request.duration_s is not None:
            payload.setdefault("duration_s", request.duration_s)
        return LyricsTimeline.from_dict(payload, strict=request.strict)


def build_lyrics_provider(cfg: Dict[str, Any]) -> LyricsProvider:
    """The provider `lyrics_alignment.provider` names (`cfg`: that section of the configuration)."""
    name = str(cfg.get("provider", "disabled")).strip().lower()
    if name in ("", "disabled", "none", "null"):
        return NullLyricsProvider("lyrics alignment disabled")
    if name == "fake":
        fixture = cfg.get("fixture_path")
        return FakeLyricsProvider(Path(str(fixture))) if fixture else NullLyricsProvider("fake lyrics provider requires fixture_path")
    if name in ("sidecar", "cli", "auto"):
        return NullLyricsProvider(_FIRERED_NOT_BUILT.format(name))
    return NullLyricsProvider(f"unsupported lyrics provider: {name}")


__all__ = ["LyricsProviderRequest", "LyricsProvider", "NullLyricsProvider", "FakeLyricsProvider", "build_lyrics_provider"]
