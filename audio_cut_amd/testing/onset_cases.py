"""Seeded cases of the `librosa_onset` mode, shared by the fixture generator (tests/golden/make_onset_golden.py) and the
tests that replay tests/golden/librosa_onset.npz: a case is a dict of seeds and parameters, `build` turns it into
(mix, vocal stem, instrumental stem).  The stems are fixed functions of the seeds, not a separation: the vocal is
`voice_with_rests * 0.5` and the instrumental is `mix - vocal`.

The seeds are the first ones (counting up from 2) whose every decision clears the generator's 1e-3 margins.  `c2_song` is
built from a few fixed loudness levels (backing only, backing + voice), so whole groups of its bars have mean RMS within
1e-5 of each other and most seeds put such a pair at a chorus threshold; the 4-min case, with four times the bars, gets a
slow seeded loudness swell (`dynamics`) that spreads the bar energies.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from . import signals

SR = signals.SR
GAPS_S = [[20.3, 21.4], [41.0, 41.8]]          # zeroed spans of the case with real silences

_C2 = {"signal": "c2_song", "duration_s": 60.0, "seed": 38, "vocal_seed": 138, "gaps_s": [], "dynamics": None, "overrides": {},
       "expect_success": True}


def _case(name: str, **changes) -> Dict:
    return dict(_C2, name=name, **changes)


CASES: List[Dict] = [
    _case("c2_60s_low"),
    _case("c2_60s_medium", overrides={"librosa_onset.density": "medium"}),
    _case("c2_60s_high", overrides={"librosa_onset.density": "high"}),
    _case("c2_60s_custom", overrides={"librosa_onset.density_custom": {"enable": True, "verse_bars": 3, "chorus_bars": 2}}),
    _case("c2_60s_gaps", gaps_s=GAPS_S),
    _case("c1_60s_fail", signal="c1_sine_silence", seed=1, vocal_seed=101, expect_success=False),
    _case("c2_60s_no_separation", overrides={"librosa_onset.use_vocal_separation": False}),
    _case("c2_240s", duration_s=240.0, seed=2, vocal_seed=102, dynamics={"depth": 0.5, "period_s": 53.0}),
    _case("c2_3s_short", duration_s=3.0, seed=2, vocal_seed=102),
]


def build(case: Dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (mix, vocal, instrumental), float32 mono at 44.1 kHz."""
    dur, seed = float(case["duration_s"]), int(case["seed"])
    mix = getattr(signals, case["signal"])(dur, seed=seed).astype(np.float32)
    dyn = case.get("dynamics")
    if dyn:         # gain between 1 - depth and 1, one swell per period, its phase from the seed
        t = np.arange(len(mix)) / float(SR)
        phase = 2 * np.pi * np.random.default_rng(seed).uniform()
        mix = (mix * (1.0 - dyn["depth"] * (0.5 + 0.5 * np.sin(2 * np.pi * t / dyn["period_s"] + phase)))).astype(np.float32)
    for a, b in case.get("gaps_s", []):
        mix[int(a * SR): int(b * SR)] = 0
    vocal = (signals.voice_with_rests(dur, seed=int(case["vocal_seed"]))[: len(mix)] * 0.5).astype(np.float32)
    inst = (mix - vocal).astype(np.float32)
    return mix, vocal, inst


__all__ = ["CASES", "GAPS_S", "build", "SR"]
