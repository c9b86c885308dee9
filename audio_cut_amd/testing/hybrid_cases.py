"""Seeded cases of the `hybrid_mdd` mode, shared by the fixture generator (tests/golden/make_hybrid_golden.py) and the tests
that replay tests/golden/hybrid_mdd.npz: a case is a dict of seeds and parameters, `build` turns it into
(mix, vocal stem, instrumental stem, beat times).

The backing is `beat_cases`' track (chord, kick on every beat, bright noise in loud chorus bars and soft verse bars).  The vocal
stem is a vibrato tone that sings everywhere except in the first `intro_s` seconds and in `gaps_s`, spans in which it falls to a
noise floor 70 dB below the voice: a beat or bar line inside a gap passes the quiet gate, one under the voice does not.  The
stems are fixed functions of the seeds, not a separation: mix = backing + vocal, instrumental = mix - vocal.  The MDD cut points
and the beats are listed, not detected: they are what the `v2.2_mdd` run and the feature cache would hand the mode.

The seeds are the first ones (counting up from 1) whose every decision clears the generator's margins.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from . import beat_cases

SR = beat_cases.SR

# chorus bars 6-9 and 16-19 of a 2 s bar grid: 12-20 s and 32-40 s
_GAPS = [[12.85, 13.15], [13.9, 14.15], [16.9, 17.15], [19.85, 20.2], [23.8, 24.2], [27.8, 28.2], [31.85, 32.2], [33.9, 34.15],
         [37.2, 37.45]]
# 5.3 verse; 12.93 -> 13.0 quiet; 14.6 -> 14.5 sung: blocked; 16.25 too far; 17.05 -> 17.0 quiet; 22.4 verse; 33.1 -> 33.0 sung;
# 34.08 -> 34.0 quiet; 37.13 -> 37.0 sung, 37.3 (the extra beat) quiet
_MDD_S = [5.3, 12.93, 14.6, 16.25, 17.05, 22.4, 33.1, 34.08, 37.13]


def _case(name: str, **kw) -> Dict:
    base = {"name": name, "duration_s": 40.0, "seed": 1, "bpm": 120.0, "bars": "VVVVVVCCCCVVVVVVCCCC", "levels": "mid",
            "extra_beats": [37.3], "beats": None, "stereo": False, "intro_s": 6.0, "gaps_s": _GAPS, "mdd_s": _MDD_S,
            "mdd_success": True, "density": None, "overrides": {"segment_layout.soft_min_s": 1.5}}
    base.update(kw)
    return base


CASES: List[Dict] = [
    _case("snap_medium"),
    _case("snap_default_min_segment", overrides={}),                                   # soft_min_s 5.0 drops cuts
    _case("snap_high", density="high"),
    _case("snap_low", density="low"),
    _case("snap_force", overrides={"segment_layout.soft_min_s": 1.5, "hybrid_mdd.chorus_force_snap": True}),
    _case("snap_unprotected", density="high", overrides={"segment_layout.soft_min_s": 1.5, "hybrid_mdd.vad_protection": False}),
    _case("beat_only_medium", overrides={"segment_layout.soft_min_s": 1.5, "hybrid_mdd.lib_alignment": "beat_only"}),
    _case("beat_only_high", density="high", overrides={"segment_layout.soft_min_s": 1.5, "hybrid_mdd.lib_alignment": "beat_only"}),
    _case("mdd_failed", mdd_success=False),
    _case("unknown_alignment", overrides={"segment_layout.soft_min_s": 1.5, "hybrid_mdd.lib_alignment": "bar_start"}),
    _case("one_beat", duration_s=20.0, beats=[1.0], extra_beats=[], bars="VVVCCCCCVV", mdd_s=[5.3, 12.93, 16.25]),
    _case("stereo_input", duration_s=30.0, stereo=True, bars="VVVVVVCCCCVVVVV", extra_beats=[], mdd_s=[5.3, 12.93, 14.6, 17.05, 22.4]),
]


def beat_times(case: Dict) -> np.ndarray:
    if case["beats"] is not None:
        return np.asarray(case["beats"], dtype=np.float64)
    period = 60.0 / float(case["bpm"])
    count = int(np.floor(float(case["duration_s"]) / period - 1e-9)) + 1
    grid = period * np.arange(count, dtype=np.float64)
    return np.sort(np.concatenate((grid, np.asarray(case["extra_beats"], dtype=np.float64))))


def mdd_cut_samples(case: Dict, n: int) -> List[int]:
    """The `cuts_samples` of the stand-in `v2.2_mdd` result: 0, the listed cuts, the end."""
    return [0] + [int(round(t * SR)) for t in case["mdd_s"] if t * SR < n] + [n]


def build(case: Dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> (mix, vocal, instrumental, beat times): float32 at 44.1 kHz, the mix mono [N] or planar stereo [2, N]."""
    backing, _ = beat_cases.build({"name": case["name"], "duration_s": case["duration_s"], "seed": case["seed"], "bpm": case["bpm"],
                                   "first_beat_s": 0.0, "n_beats": None, "bars": case["bars"], "levels": case["levels"],
                                   "stereo": False, "beats": None, "time_signature": 4})
    n = len(backing)
    rng = np.random.default_rng(1000 + int(case["seed"]))
    t = np.arange(n) / float(SR)
    sing = np.ones(n)
    sing[: int(float(case["intro_s"]) * SR)] = 0.0
    for a, b in case["gaps_s"]:
        sing[int(a * SR): int(b * SR)] = 0.0
    voice = 0.2 * np.sin(2 * np.pi * 330.0 * t + 1.5 * np.sin(2 * np.pi * 5.5 * t)) * (1.0 + 0.3 * np.sin(2 * np.pi * 1.3 * t))
    vocal = (sing * voice + 6e-5 * rng.standard_normal(n)).astype(np.float32)
    mono = (backing + vocal).astype(np.float32)
    inst = (mono - vocal).astype(np.float32)
    beats = beat_times(case)
    if not case["stereo"]:
        return mono, vocal, inst, beats
    side = (0.05 * np.sin(2 * np.pi * 0.31 * t) * backing).astype(np.float32)
    return np.stack([mono + side, mono - side]).astype(np.float32), vocal, inst, beats


def mono_of(mix: np.ndarray) -> np.ndarray:
    """The mix the mode cuts: the track itself, or the float32 (L + R) * 0.5 of a stereo one."""
    return mix if mix.ndim == 1 else (mix[0] + mix[1]) * np.float32(0.5)


__all__ = ["CASES", "SR", "build", "beat_times", "mdd_cut_samples", "mono_of"]
