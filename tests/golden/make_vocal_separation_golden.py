#!/usr/bin/env python3
"""Generate tests/golden/vocal_separation.json by running the reference's own `_process_vocal_separation_only`
(`src/vocal_smart_splitter/core/seamless_splitter.py:958-1036`) and `_build_manifest` (`src/audio_cut/api.py:178-263`).

Runs ONLY where the reference exists; the GPU box never sees it.  As in make_hybrid_golden.py, `oracle.librosa_ops` is registered
under the name `librosa` (make_beat_golden.py does that and sets the paths) and the splitter is built with `object.__new__`: the
track loader returns a fixed mix, the separator fixed stems, and the exporter writes nothing and returns the path `export_audio`
would have written (`utils/audio_export.py:70-90`: the base name keeps its dot, the extension is appended).

The fixture holds data only: per case the export plan handed in, the result's key set, `method`, `num_segments`, `export_plan`,
the base names of the files, and the manifest's `artifacts` / `cuts` / `stats` / `segments` blocks with the output directory
written as `$OUT` (not the duration: the reference reads it from the file header through soundfile, which is a stub here).  The
cases: no plan, `['full_vocal']`, a plan with a segment kind in it, a plan of a segment kind alone, and
a separation without an instrumental.
"""
from __future__ import annotations

import json
import sys
import tempfile
import types
import wave
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_beat_golden as MB  # noqa: E402,F401  (registers the librosa stand-in, sets the paths)

from audio_cut import api as ref_api  # noqa: E402
from vocal_smart_splitter.core import seamless_splitter as ref_ss  # noqa: E402

SR = 44100
N = int(7.26 * SR)
NAME = "song"
GPU_META = {"gpu_pipeline_used": True, "gpu_pipeline_processed_chunks": 1}
CASES = [
    {"name": "default", "export_plan": None, "instrumental": True},
    {"name": "vocal_only", "export_plan": ["full_vocal"], "instrumental": True},
    {"name": "with_segment_kind", "export_plan": ["full_instrumental", "mix_segments"], "instrumental": True},
    {"name": "segment_kind_alone", "export_plan": ["vocal_segments"], "instrumental": True},
    {"name": "no_instrumental", "export_plan": None, "instrumental": False},
]


def run_reference(case, src: Path, out_dir: Path):
    rng = np.random.default_rng(5)
    mix = (0.2 * rng.standard_normal(N)).astype(np.float32)
    vocal = (0.1 * rng.standard_normal(N)).astype(np.float32)
    inst = mix - vocal if case["instrumental"] else None
    fake = object.__new__(ref_ss.SeamlessSplitter)
    fake.sample_rate = SR
    fake._export_format = "wav"
    fake._export_options = {}
    fake._precision_guard_ok = True
    fake._last_guard_shift_stats = fake._blank_guard_stats()
    fake._load_and_resample_if_needed = lambda path: mix
    fake.separator = types.SimpleNamespace(separate_for_detection=lambda audio: types.SimpleNamespace(
        vocal_track=vocal, instrumental_track=inst, backend_used="seeded", separation_confidence=0.625, gpu_meta=dict(GPU_META)))
    fake.segment_exporter = types.SimpleNamespace(
        export_full_track=lambda audio, base, **k: str(Path(base).parent / f"{Path(base).name}.{k['export_format']}"))
    res = fake._process_vocal_separation_only(str(src), str(out_dir), export_plan=case["export_plan"])
    man = ref_api._build_manifest(result=res, input_path=src, export_dir=out_dir, mode="vocal_separation", sample_rate=SR, channels=1,
                                  layout_cfg={})
    return res, man


def main() -> None:
    out = {"sample_rate": SR, "n_samples": N, "input_name": NAME, "gpu_meta": GPU_META, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / f"{NAME}.wav"
        with wave.open(str(src), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(np.zeros(N, "<i2").tobytes())
        out_dir = Path(tmp) / "out"
        out_dir.mkdir()
        for case in CASES:
            res, man = run_reference(case, src, out_dir)
            base = lambda p: None if p is None else Path(p).name
            text = json.dumps({k: man[k] for k in ("artifacts", "cuts", "stats", "segments", "export_plan")}).replace(out_dir.as_posix(), "$OUT")
            row = dict(case, result_keys=sorted(res), success=res["success"], method=res["method"], num_segments=res["num_segments"],
                       result_export_plan=res["export_plan"], saved_files=[base(p) for p in res["saved_files"]],
                       full_vocal_file=base(res["full_vocal_file"]), full_instrumental_file=base(res["full_instrumental_file"]),
                       mix_segment_files=res["mix_segment_files"], vocal_segment_files=res["vocal_segment_files"],
                       segment_durations=res["segment_durations"], guard_shift_stats=res["guard_shift_stats"],
                       precision_guard_ok=res["precision_guard_ok"], precision_guard_threshold_ms=res["precision_guard_threshold_ms"],
                       separation_confidence=res["separation_confidence"], backend_used=res["backend_used"],
                       manifest=json.loads(text))
            print(f"  {case['name']}: plan {res['export_plan']}  files {row['saved_files']}  artifacts {sorted(row['manifest']['artifacts'])}")
            out["cases"].append(row)
    path = HERE / "vocal_separation.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"wrote {path.name} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
