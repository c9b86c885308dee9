"""Controlled failures of the lyrics layer (reference `src/audio_cut/exceptions.py`): what a caller may catch by class."""


class AudioCutError(Exception):
    """Base class of the failures this library raises on purpose."""


class LyricsAlignmentUnavailable(AudioCutError):
    """Lyrics alignment was asked for and no provider can supply it."""


class TimelineValidationError(AudioCutError):
    """A lyrics timeline holds invalid or inconsistent timestamps."""


__all__ = ["AudioCutError", "LyricsAlignmentUnavailable", "TimelineValidationError"]
