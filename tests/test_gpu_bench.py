"""bench.py's plain run on the GPU: --steps sets the timed steps, the line carries the headline fields and
none of what --full measures, and --dump-outputs writes the last timed step's outputs as float32 .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


B, MU = 8, 7  # the per-rank shard of N = 8: the F1 batch split eight ways


def _bench(steps, warmup, *extra):
    """One `bench.py --gpus 1` run at the B = 8 shard; its one JSON line, the headline fields checked."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--batch", str(B), "--mu", str(MU), *extra],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == warmup and line["higher_is_better"] is True
    assert line["unit"] == "unlabeled images/s" and line["dtype"] == "bf16"
    # value and ms_per_step describe the same timed steps: B * mu unlabeled images per step
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - B * MU) <= 1e-3 * B * MU
    return line


def test_full_run_adds_roofline_and_counts_timed_steps():
    """--full (without the CPU baseline): the roofline of the dominant launch, live in the 3 timed steps and
    isolated, and mfma_util.  The live events are recorded in the timed steps alone, so their count says how
    many steps the timed loop ran: at this shard (M = 12,608 train tokens < Engine.GROUP_WGRAD_MAX_M) the
    backward sends its weight gradients as grouped launches, one at every block i > 0 with
    i % Engine.GROUP_LAYERS == 0 and one after the patch embedding (Engine.backward)."""
    from endossl.vit import Engine, ViTConfig
    assert Engine.GROUP_WGRAD == "auto" and B * (1 + MU) * 197 < Engine.GROUP_WGRAD_MAX_M
    per_step = sum(1 for i in range(1, ViTConfig().depth) if i % Engine.GROUP_LAYERS == 0) + 1
    line = _bench(3, 1, "--full", "--no-cpu-baseline")
    rl = line["roofline"]
    assert rl["timed"].startswith("live in the timed steps") and rl["kernel"].startswith("es_gemm_tn_grouped")
    assert rl["launches"] == 3 * per_step
    assert rl["mean_launch_ms"] > 0 and 0 < rl["frac"] < 1
    assert rl["isolated"]["mean_launch_ms"] > 0 and 0 < rl["isolated"]["frac"] < 1
    assert "mfma_util" in line and "cpu_baseline" not in line


def test_plain_run_line_and_dumped_outputs(tmp_path):
    """One plain run, 2 timed steps after 1 warm-up step."""
    line = _bench(2, 1, "--dump-outputs", str(tmp_path / "dump"))
    for k in ("roofline", "mfma_util", "cpu_baseline", "weak_scaling", "allreduce_other_form"):
        assert k not in line, k  # --full only
    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == sorted(n + ".npy" for n in ("loss", "lx", "lu", "mask_mean", "pseudo_label", "mask", "grad",
                                                 "weights", "ema_weights"))
    arrs = {f[:-4]: np.load(tmp_path / "dump" / f, allow_pickle=False) for f in files}
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10**6
    for name, a in arrs.items():
        assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), name
    assert arrs["pseudo_label"].shape == (B * MU,) and arrs["mask"].shape == (B * MU,)
    assert set(np.unique(arrs["mask"])) <= {0.0, 1.0}
    assert ((arrs["pseudo_label"] >= 0) & (arrs["pseudo_label"] < 23)).all()
    assert abs(float(arrs["loss"][0]) - line["final_loss"]) <= 1e-6  # the line rounds to 6 places
    assert arrs["grad"].shape == arrs["weights"].shape == arrs["ema_weights"].shape == (4_000_000,)
    assert np.abs(arrs["grad"]).max() > 0 and np.abs(arrs["weights"] - arrs["ema_weights"]).max() > 0
