"""bench.py's contract on the GPU: a plain run (`--gpus 1 --steps K --warmup W`) times K decode steps and prints the
headline line only -- nothing of what `--full` adds -- and `--dump-outputs DIR` writes what the last timed step
computed.  One short run of the benchmark (a child process: that is what is under test), shared by the tests.

The dumped logits are checked against the same lm_head launch made here: same seeded weight, same seeded input, same
kernel, so they agree within fp32 reassociation, 1e-5 of max|logits| (the bar tests/test_oracle_golden.py uses for
two summation orders of one GEMV)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 1
FULL_ONLY = ("decode_eager_tokens_per_s", "prefill_tflops", "roofline", "per_op_launches", "prefill_roofline",
             "synthetic", "workloads", "cpu_baseline")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", str(out)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), out


def test_plain_run_prints_the_headline_only(plain_run):
    line, _ = plain_run
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["n_gpus"] == 1 and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = steps / dt and ms_per_step = dt / steps, each rounded (2 and 4 decimals)
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) <= 1e-3
    assert not [k for k in FULL_ONLY if k in line]


def test_dump_outputs_hold_the_last_step(plain_run):
    import bench
    _, out = plain_run
    H, V = bench.LLAMA["hidden"], bench.LLAMA["vocab"]
    shapes = {"qkv": (3, 1, H), "o": (1, H), "ffn": (1, H), "logits": (1, V)}
    assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in shapes)
    arrays = {n: np.load(out / f"{n}.npy") for n in shapes}
    for n, a in arrays.items():
        assert a.dtype == np.float32 and a.shape == shapes[n], n
        assert np.isfinite(a).all() and np.abs(a).max() > 0, n
    # lm_head and the input row do not depend on the layer count: a one-layer stack makes the same launch
    st = bench.Stack(dict(bench.LLAMA, layers=1), 0, 1)
    run = bench.Runner(st, 1, None, "cuda")
    run.step()
    ref = run.outputs()["logits"].cpu().numpy()
    assert np.abs(arrays["logits"] - ref).max() <= 1e-5 * np.abs(ref).max()
