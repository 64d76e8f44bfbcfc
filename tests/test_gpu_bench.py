"""GPU (-m gpu): what a plain `bench.py` line holds and what `--full` adds.  A plain run times the steps and prints the
headline only; the CPU baseline with its oracle parity check and the other operand formats run under `--full` alone.
Small batch (2 images), so neither run is a figure of record."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline")
FULL_ONLY = ("cpu_baseline", "parity", "f32x3_path", "bf16_path", "train_bf16_path", "l16_1024_tiled_f16_path",
             "serve_path", "ref_grid_path")


def _line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "2", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def test_plain_line_is_the_headline_only():
    out = _line()
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in out], sorted(out)


def test_full_line_adds_cpu_baseline_parity_and_other_formats():
    out = _line("--full")
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["cpu_baseline"]["value"] > 0 and out["parity"]["images_checked"] == 2
    assert out["parity"]["mask_mismatch_at_stable_pixels"] == 0
    assert out["f32x3_path"]["parity_vs_oracle"]["mask_mismatch_at_stable_pixels"] == 0
    assert out["bf16_path"]["ms_per_step"] > 0
