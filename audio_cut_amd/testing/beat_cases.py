"""Seeded cases of the beat / bar analysis layer, shared by the fixture generator (tests/golden/make_beat_golden.py) and the
tests that replay tests/golden/beat_analysis.npz: a case is a dict of seeds and parameters, `build` turns it into
(track, beat times).  The beats are given, not detected: they are what a feature cache would hand the analyser.

A track is a chord, a kick on every beat and first-differenced (bright) noise, laid out in verse and chorus bars; either
kind has a level and a brightness, and every bar gets a small seeded deviation of both so that no two bars tie.  The
spread of the two levels puts the coefficient of variation of the bar energies into one of the three regimes the
chorus fusion distinguishes (`cv` < 0.15, between, > 0.4).

The seeds are the first ones (counting up from 1) whose every decision clears the generator's 1e-3 margins.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

SR = 44100

# (level, brightness) of a verse (V) and a chorus (C) bar
_LOW = {"V": (0.92, 0.15), "C": (1.0, 1.0)}        # loudness hardly moves, the spectrum does
_MID = {"V": (0.55, 0.3), "C": (1.0, 1.0)}
_HIGH = {"V": (0.12, 0.6), "C": (1.0, 1.0)}


def _case(name: str, **kw) -> Dict:
    base = {"name": name, "duration_s": 40.0, "seed": 1, "bpm": 120.0, "first_beat_s": 0.0, "n_beats": None,
            "bars": "VVVVVVCCCCVVVVVVCCCC", "levels": "mid", "stereo": False, "beats": None, "cache_bpm": None,
            "hop_length": 512, "time_signature": 4, "energy_percentile": 70.0}
    base.update(kw)
    return base


# `bars`: the kind of every bar of the TRACK's own grid (first beat, bpm), repeated if the track is longer.  Four bars in ten are
# chorus bars, the share the fused 60th percentile lets through, in runs of at least four.
CASES: List[Dict] = [
    _case("mid_two_choruses", levels="mid", seed=3),
    _case("low_dynamics", levels="low", seed=3, cache_bpm=120.0),
    _case("high_dynamics", levels="high", duration_s=60.0, bars="VVVVVVCCCCVVVVVCCCCVVVVVCCCCVV"),
    _case("partial_last_bar", levels="mid", duration_s=33.3, bpm=96.0, first_beat_s=0.37, n_beats=46, bars="VVVCCCCCVVVV"),
    _case("few_beats_grid", levels="mid", duration_s=20.0, beats=[0.5, 1.1, 1.7], bars="VVVCCCCCVV"),
    _case("stereo_input", levels="high", duration_s=30.0, stereo=True, bars="VVVVCCCCCCVVVVV", energy_percentile=60.0),
]

_LEVELS = {"low": _LOW, "mid": _MID, "high": _HIGH}


def beat_times(case: Dict) -> np.ndarray:
    if case["beats"] is not None:
        return np.asarray(case["beats"], dtype=np.float64)
    period = 60.0 / float(case["bpm"])
    count = case["n_beats"]
    if count is None:
        count = int(np.floor((float(case["duration_s"]) - float(case["first_beat_s"])) / period - 1e-9)) + 1
    return float(case["first_beat_s"]) + period * np.arange(int(count), dtype=np.float64)


def build(case: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """-> (track float32, mono [N] or planar stereo [2, N], at 44.1 kHz; beat times in seconds, float64)."""
    rng = np.random.default_rng(int(case["seed"]))
    n = int(round(float(case["duration_s"]) * SR))
    t = np.arange(n) / float(SR)
    beats = beat_times(case)
    period = 60.0 / float(case["bpm"])
    bar_s = period * int(case["time_signature"])
    first = float(case["first_beat_s"])
    n_bars = int(np.ceil((float(case["duration_s"]) - first) / bar_s)) + 1
    table = _LEVELS[case["levels"]]
    level = np.empty(n_bars); bright = np.empty(n_bars)
    for b in range(n_bars):
        kind = case["bars"][b % len(case["bars"])]
        lv, br = table[kind]
        level[b] = lv * (1.0 + 0.06 * rng.uniform(-1.0, 1.0))
        bright[b] = br * (1.0 + 0.15 * rng.uniform(-1.0, 1.0))
    bar_of = np.clip(np.floor((t - first) / bar_s).astype(int), 0, n_bars - 1)
    chord = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in
                ((220.0, 0.12, 0.0), (277.18, 0.09, 0.7), (329.63, 0.08, 1.9), (440.0, 0.05, 2.4)))
    kick = np.zeros(n)
    k_len = int(0.12 * SR)
    k_t = np.arange(k_len) / float(SR)
    k_wave = 0.35 * np.sin(2 * np.pi * 62.0 * k_t) * np.exp(-k_t / 0.03)
    for bt in np.arange(first, float(case["duration_s"]), period):
        i = int(round(bt * SR))
        m = min(k_len, n - i)
        if m > 0:
            kick[i: i + m] += k_wave[:m]
    hats = np.diff(rng.standard_normal(n + 1)) * 0.05                 # first difference: energy towards the top of the band
    mono = level[bar_of] * (chord + kick + bright[bar_of] * hats)
    if not case["stereo"]:
        return mono.astype(np.float32), beats
    side = 0.08 * np.sin(2 * np.pi * 0.31 * t) * chord
    return np.stack([mono + side, mono - side]).astype(np.float32), beats


def cache_for(case: Dict, beats: np.ndarray):
    """What `analyze_beats` reads of a feature cache: the beat times and, where the case has one, the cached BPM."""
    import types
    bpm = None if case["cache_bpm"] is None else types.SimpleNamespace(main_bpm=float(case["cache_bpm"]))
    return types.SimpleNamespace(beat_times=np.asarray(beats, dtype=np.float64), bpm_features=bpm)


__all__ = ["CASES", "SR", "build", "beat_times", "cache_for"]
