"""Seeded lyrics timelines over `vpbd_inputs.vpbd_case` (tests + golden generation for mode `vpbd_asr`): what a provider could
return for that case's track, in the layout of `LyricsTimeline.to_dict()` / the `fake` provider's fixture file.

A timeline is laid out between some of the case's own pauses, so that sentence ends, word gaps and region edges fall near
acoustic candidates (clusters that merge a lyrics and an acoustic candidate) as well as far from them.  It covers:
  * word gaps below 0.35 s (no candidate), between 0.35 s and 1.5 s, and beyond 1.5 s (score saturates);
  * word confidences None, >= 0.85 and below (the three weights of the inside-word penalty);
  * sentences with and without terminal punctuation, one of them CJK with a full-width stop (joined without spaces);
  * `vad_regions` of kind `singing` (penalised) and of other kinds (ignored by the penalty, still boundary candidates).
All times are whole milliseconds, as ASR engines report them."""
from __future__ import annotations

from typing import Any, Dict, List

import numpy as np

from .vpbd_inputs import vpbd_case

_LATIN = ("la", "day", "light", "over", "river", "home", "again", "slow", "burn", "heart", "run", "away", "night", "fall", "we")
_CJK = ("你", "好", "世", "界", "再", "见")
_ENDINGS = (".", "", "!", "", "?", "")


def _ms(v: float) -> float:
    return round(float(v), 3)


def lyrics_case(seed: int, duration: float = 60.0) -> Dict[str, Any]:
    """-> the timeline payload (`duration_s`, `source`, `words`, `sentences`, `vad_regions`) of `vpbd_case(seed, duration)`."""
    _, pauses, _ = vpbd_case(seed, duration)
    rng = np.random.default_rng(7000 + seed)
    anchors: List[float] = [0.6]
    for p in pauses:                                    # sentence boundaries sit at pauses at least 2.5 s apart
        if p.cut_point - anchors[-1] >= 2.5 and p.cut_point < duration - 2.5:
            anchors.append(float(p.cut_point))
    anchors.append(duration - 0.8)
    words: List[Dict[str, Any]] = []
    sentences: List[Dict[str, Any]] = []
    regions: List[Dict[str, Any]] = []
    conf_cycle = (None, "high", "low")
    lead = (0.05, 0.25, 0.9, 1.4)                       # silence after / before an anchor: sentence gaps from 0.1 s to 2.8 s
    n_word = 0
    for i, (a, b) in enumerate(zip(anchors[:-1], anchors[1:])):
        if i % 7 == 5:                                  # an instrumental stretch: no lyrics, one region of another kind
            regions.append({"start_s": _ms(a + 0.3), "end_s": _ms(b - 0.3), "confidence": _ms(rng.uniform(0.5, 0.95)), "kind": "music"})
            continue
        start = _ms(a + lead[int(rng.integers(0, 4))])
        end = _ms(b - lead[int(rng.integers(0, 4))])
        if end - start < 0.8:
            continue
        cjk = i == 2
        vocab = _CJK if cjk else _LATIN
        t, first = start, len(words)
        while True:
            dur = float(rng.uniform(0.2, 0.6))
            if t + dur > end - 0.15:                    # the last word runs to the sentence end
                dur = end - t
            kind = conf_cycle[n_word % 3]
            conf = None if kind is None else _ms(rng.uniform(0.87, 0.99) if kind == "high" else rng.uniform(0.35, 0.83))
            words.append({"text": vocab[n_word % len(vocab)], "start_s": _ms(t), "end_s": _ms(t + dur), "confidence": conf})
            n_word += 1
            if _ms(t + dur) >= end:
                break
            gap = float(rng.uniform(0.03, 0.30) if rng.random() < 0.75 else rng.uniform(0.40, 0.90))
            t = _ms(t + dur + gap)
            if end - t < 0.2:                           # no room for another word: stretch the last one
                words[-1]["end_s"] = end
                break
        mine = words[first:]
        text = ("" if cjk else " ").join(w["text"] for w in mine) + ("。" if cjk else _ENDINGS[i % len(_ENDINGS)])
        sentences.append({"text": text, "start_s": mine[0]["start_s"], "end_s": mine[-1]["end_s"],
                          "confidence": None if i % 4 == 1 else _ms(rng.uniform(0.6, 0.98))})
        regions.append({"start_s": _ms(max(0.0, mine[0]["start_s"] - 0.05)), "end_s": _ms(min(duration, mine[-1]["end_s"] + 0.08)),
                        "confidence": (None, _ms(rng.uniform(0.86, 0.97)), _ms(rng.uniform(0.4, 0.8)))[i % 3],
                        "kind": "speech" if i % 5 == 3 else "singing"})
    return {"duration_s": float(duration), "source": "fake", "words": words, "sentences": sentences, "vad_regions": regions}


CASE_SECONDS = 20.0


def asr_case(seed: int, breaths: bool = False, seconds: float = CASE_SECONDS):
    """-> (cache, pauses, vocal, timeline payload): `vpbd_case(seed, seconds)` with every fourth of its pauses (a pool a reader can
    follow) and `lyrics_case(seed, seconds)`; with `breaths` every second pause kept is a breath (`pause_type="breath"`: the unified
    pool re-labels it as a `breath` candidate and scales its score)."""
    cache, pauses, vocal = vpbd_case(seed, seconds)
    pauses = pauses[::4]
    if breaths:
        for p in pauses[1::2]:
            p.pause_type = "breath"
    return cache, pauses, vocal, lyrics_case(seed, seconds)


__all__ = ["lyrics_case", "asr_case", "CASE_SECONDS"]
