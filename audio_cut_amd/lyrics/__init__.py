"""The lyrics layer of mode `vpbd_asr`: the timeline model, the provider seam, the candidate generator and the segment
attachment (reference `src/audio_cut/lyrics/`).  Host code over a few hundred words per track.  The ASR engines themselves
(FireRed sidecar / CLI, their protocol, chunker, chunk merge and cache) are external processes and are not built here: a host
application plugs its own engine in at `LyricsProvider.align` (`vpbd_asr`)."""
from .candidates import LyricsBoundaryCandidateGenerator
from .models import LyricsTimeline, Sentence, VadRegion, Word
from .providers import (FakeLyricsProvider, LyricsProvider, LyricsProviderRequest, NullLyricsProvider, build_lyrics_provider)
from .segment_attach import attach_lyrics_to_segments

__all__ = ["LyricsBoundaryCandidateGenerator", "LyricsTimeline", "Sentence", "VadRegion", "Word", "FakeLyricsProvider",
           "LyricsProvider", "LyricsProviderRequest", "NullLyricsProvider", "build_lyrics_provider", "attach_lyrics_to_segments"]
