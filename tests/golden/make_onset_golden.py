#!/usr/bin/env python3
"""Generate tests/golden/librosa_onset.npz by running the reference's own `_process_librosa_onset_split`
(`src/vocal_smart_splitter/core/seamless_splitter.py:1038-1349`) over the oracle's librosa restatement.

Runs ONLY where the reference exists (/root/reference); the GPU box never sees it.  As in make_golden.py,
`oracle.librosa_ops` is registered under the name `librosa`, `soundfile` / `pydub` are stubbed, and the splitter is built
with `object.__new__` (its constructor would load models): the track loader returns the seeded track, the separator returns
seeded stems, the exporter writes nothing and the result builder returns its keyword arguments.

The method's locals that the result does not carry are observed, not restated: the RMS series is what `librosa.feature.rms`
returned and the bar energies are what the method passed to `np.percentile`.

The fixture holds data only - seeds, parameters, effective config, and per case tempo, bar duration, bar energies, bar types,
silence boundaries, cut samples and flags - never a track or a stem.  The product reproduces the float series only to
tolerance (README: 1e-4), so before anything is written every decision taken on such a series must clear its threshold by
1e-3, ten times that tolerance:
  * every bar energy that is not bit-equal to a percentile threshold: |energy - thr| / thr >= 1e-3, for both thresholds;
  * every RMS frame: |20 log10(rms + 1e-10) - threshold_db| >= 1e-3 dB;
  * every segment: |vocal_rms - 0.3 inst_rms| / (0.3 inst_rms) >= 1e-3.
A case that misses a margin gets another seed, never a smaller margin.  The minima are stored (`min_margin_*`).
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np
import scipy

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
REF = Path("/root/reference")
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(REF / "src"))

from oracle import librosa_ops  # noqa: E402

librosa_ops.install_as_librosa()
for _name in ("soundfile", "pydub"):
    if _name not in sys.modules:
        sys.modules[_name] = types.ModuleType(_name)
sys.modules["pydub"].AudioSegment = object  # type: ignore[attr-defined]

from audio_cut_amd.cutting import smart_segment as SS  # noqa: E402
from audio_cut_amd.testing import onset_cases  # noqa: E402
from vocal_smart_splitter.core import seamless_splitter as ref_ss  # noqa: E402
from vocal_smart_splitter.utils import config_manager as ref_cfg  # noqa: E402

VERSIONS = {"numpy": np.__version__, "scipy": scipy.__version__}
SR = 44100
MARGIN = 1e-3


class _NumpyTap:
    """`numpy` as the reference module sees it, with `percentile` recording its first argument."""

    def __init__(self):
        self.percentile_inputs = []

    def __getattr__(self, name):
        return getattr(np, name)

    def percentile(self, a, q, *args, **kwargs):
        self.percentile_inputs.append(list(a))
        return np.percentile(a, q, *args, **kwargs)


def run_reference(mix: np.ndarray, vocal, inst):
    """-> (result dict, RMS series the method computed, bar energies it formed)."""
    fake = object.__new__(ref_ss.SeamlessSplitter)
    fake.sample_rate = SR
    fake._export_format = "wav"
    fake._export_options = {}
    fake._load_and_resample_if_needed = lambda path: mix
    fake.separator = types.SimpleNamespace(
        separate_for_detection=lambda audio: types.SimpleNamespace(vocal_track=vocal, instrumental_track=inst))
    fake.segment_exporter = types.SimpleNamespace(export_segments=lambda *a, **k: [])
    fake.result_builder = types.SimpleNamespace(build_base=lambda **k: dict(k), add_separation_metadata=lambda r, s: r)
    tap = _NumpyTap()
    seen = {}
    real_rms = ref_ss.librosa.feature.rms

    def rms_tap(*a, **k):
        seen["rms"] = real_rms(*a, **k)
        return seen["rms"]

    ref_ss.np = tap
    ref_ss.librosa.feature.rms = rms_tap
    try:
        res = fake._process_librosa_onset_split("track.wav", "/nonexistent", export_plan=("mix_segments",))
    finally:
        ref_ss.np = np
        ref_ss.librosa.feature.rms = real_rms
    energies = tap.percentile_inputs[0] if tap.percentile_inputs else []
    return res, np.asarray(seen["rms"][0]), energies


def margins(case, res, rms, energies, lo_cfg, vocal, inst):
    thr_db = float(lo_cfg["silence"]["threshold_db"])
    db = 20.0 * np.log10(rms.astype(np.float64) + 1e-10)
    m_db = float(np.min(np.abs(db - thr_db)))
    e = np.asarray(energies, dtype=np.float64)
    ea = lo_cfg["energy_analysis"]
    m_bar = np.inf
    for pct in (ea.get("chorus_percentile", 60), ea.get("chorus_peak_percentile", 80)):
        thr = float(np.percentile(energies, pct))
        off = e[e != thr]
        if off.size:
            m_bar = min(m_bar, float(np.min(np.abs(off - thr) / thr)))
    m_seg = np.inf
    cuts = res["cut_points_samples"]
    if lo_cfg["use_vocal_separation"]:
        for a, b in zip(cuts[:-1], cuts[1:]):
            v = float(np.sqrt(np.mean(vocal[a:b].astype(np.float64) ** 2)))
            i = 0.3 * float(np.sqrt(np.mean(inst[a:b].astype(np.float64) ** 2)))
            m_seg = min(m_seg, abs(v - i) / i)
    print(f"  {case['name']}: margins  frame {m_db:.3e} dB   bar {m_bar:.3e}   segment {m_seg:.3e}")
    assert m_db >= MARGIN, (case["name"], "silence margin", m_db)
    assert m_bar >= MARGIN, (case["name"], "bar margin", m_bar)
    assert m_seg >= MARGIN, (case["name"], "segment margin", m_seg)
    return m_db, m_bar, m_seg


def main() -> None:
    out = {}
    listing = []
    effective = None
    mins = [np.inf, np.inf, np.inf]
    by_name = {}
    for case in onset_cases.CASES:
        ref_cfg.reset_runtime_config()
        ref_cfg.set_runtime_config(dict(case["overrides"]))
        try:
            lo_cfg = ref_cfg.get_librosa_onset_config()
            soft_min = float(ref_cfg.get_config("segment_layout.soft_min_s", 2.0))
            if not case["overrides"]:
                effective = {"librosa_onset": lo_cfg, "segment_layout.soft_min_s": soft_min}
            mix, vocal, inst = onset_cases.build(case)
            name = case["name"]
            if not case["expect_success"]:
                # the dispatcher's failure result (`:231-233`) for what the method raises
                try:
                    run_reference(mix, vocal, inst)
                    raise AssertionError(f"{name}: expected the reference to fail")
                except ZeroDivisionError as exc:
                    listing.append(dict(case, success=False, error=str(exc)))
                    print(f"  {name}: reference fails with {exc!r}")
                continue
            res, rms, energies = run_reference(mix, vocal, inst)
        finally:
            ref_cfg.reset_runtime_config()
        m = margins(case, res, rms, energies, lo_cfg, vocal, inst)
        mins = [min(a, b) for a, b in zip(mins, m)]
        # the product's pure host rules, fed the reference's series, must give the reference's cuts
        bar_types, _, _ = SS.classify_bars(energies, lo_cfg["energy_analysis"]["chorus_percentile"],
                                           lo_cfg["energy_analysis"]["chorus_peak_percentile"])
        duration = len(mix) / float(SR)
        times = SS.plan_bar_cuts(SS.bar_grid(duration, res["bar_duration_s"]), bar_types, res["silence_boundaries"],
                                 SS.density_config(lo_cfg), duration, soft_min)
        assert SS.to_sample_points(times, SR, len(mix)) == list(res["cut_points_samples"]), name
        assert res["method"] == "smart_segment_v2" and res["use_vocal_preprocessing"] == lo_cfg["use_vocal_separation"]
        listing.append(dict(case, success=True, density=res["density"], n_samples=len(mix), soft_min_s=soft_min))
        out[f"{name}__scalars"] = np.array([res["bpm"], res["bar_duration_s"]], dtype=np.float64)
        out[f"{name}__bar_energies"] = np.asarray(energies, dtype=np.float64)
        out[f"{name}__bar_types"] = np.array([SS_TYPE_CODE[t] for t in bar_types], dtype=np.int8)
        out[f"{name}__silence_boundaries"] = np.asarray(res["silence_boundaries"], dtype=np.float64)
        out[f"{name}__cuts"] = np.asarray(res["cut_points_samples"], dtype=np.int64)
        out[f"{name}__flags"] = np.asarray(res["segment_vocal_flags"], dtype=bool)
        by_name[name] = res
        print(f"  {name}: bpm {res['bpm']!r} cuts {list(res['cut_points_samples'])} flags {list(res['segment_vocal_flags'])} "
              f"silences {res['silence_boundaries']}")
    gap, plain = by_name["c2_60s_gaps"], by_name["c2_60s_low"]
    assert len(gap["silence_boundaries"]) >= 2, gap["silence_boundaries"]
    assert list(gap["cut_points_samples"]) != list(plain["cut_points_samples"])
    assert len(set(plain["segment_vocal_flags"])) == 2, "both labels must occur in the low-density case"
    for preset in ("c2_60s_low", "c2_60s_medium", "c2_60s_high"):       # the custom bar counts must show in the cuts
        assert list(by_name["c2_60s_custom"]["cut_points_samples"]) != list(by_name[preset]["cut_points_samples"]), preset
    path = HERE / "librosa_onset.npz"
    np.savez_compressed(path, versions=json.dumps(VERSIONS), cases=json.dumps(listing), effective_config=json.dumps(effective),
                        min_margin_frame_db=mins[0], min_margin_bar_rel=mins[1], min_margin_segment_rel=mins[2], **out)
    print(f"wrote {path.name} ({path.stat().st_size} bytes); min margins: frame {mins[0]:.3e} dB, bar {mins[1]:.3e}, "
          f"segment {mins[2]:.3e}")


SS_TYPE_CODE = {"verse": 0, "chorus": 1, "chorus_peak": 2}

if __name__ == "__main__":
    main()
