"""bench.py on the hardware: a plain run prints the headline line and nothing it does not need; --full still runs every side-line and
check that moved behind it (small sizes here: the point is that each block runs and reports, not its figures)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "rccl", "per_rank_hist_mass")
FULL_ONLY = ("roofline", "roofline_par_iterate", "roofline_vit_cam", "roofline_sim_gemm", "kernel_ms_per_step", "cpu_baseline", "verify",
             "numerics_check", "power", "checkpoint_like_weights", "harness_ragged")


def _bench(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"] + args,
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                            # ONE JSON line
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline():
    """Default side-line sizes, no --full: the line has the headline and none of the side-line blocks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _bench([], timeout=600)
    assert all(k in out for k in HEADLINE), out.keys()
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["rccl_ranks"] == 1
    assert abs(out["value"] - 32 / (out["ms_per_step"] * 1e-3)) < 1e-2 * out["value"]


@pytest.mark.timeout(1200)
def test_bench_full_runs_every_sideline():
    """--full with small side-lines: every block is in the line, and the label checks against the CPU port passed (exit status 0)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _bench(["--full", "--cpu-images", "4", "--ragged-images", "32", "--power-seconds", "0.5", "--fp16w-steps", "2"], timeout=1200)
    assert all(k in out for k in HEADLINE + FULL_ONLY), [k for k in HEADLINE + FULL_ONLY if k not in out]
    assert out["verify"]["images"] == 4 and out["verify"]["label_agreement_mean"] >= 0.999
    assert out["checkpoint_like_weights"]["verify"]["label_agreement_mean"] >= 0.999
    assert out["harness_ragged"]["images"] == 32 and out["harness_ragged"]["hist_equal_resident_vs_decoded"]
    assert out["roofline"]["achieved"] > 0 and sum(out["kernel_ms_per_step"].values()) > 0
