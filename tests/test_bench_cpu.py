"""bench.py's contract on CPU (no GPU): `--gpus 8 --dry-run` prints the per-rank tensor-parallel shard table the
8-GPU run would build, following docs/tensor_parallelism.md's split and the reference's loader
(model_files.h:134-235): Q/K/V column shards are whole heads, O / down are split along K by the same boundaries as the
columns feeding them, and down's K shards are whole quantization groups -- Llama-2-7B F = 11008 = 86 groups of 128 ->
11 groups on ranks 0-5 and 10 on ranks 6-7 (the reference itself requires even splits; here they are exact)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dry(gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(gpus), "--dry-run"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dry_run_tp8_shard_table():
    d = _dry(8)
    assert d["relaunch"] and d["nproc_per_node"] == 8
    rows = d["shards"]
    assert [r["rank"] for r in rows] == list(range(8))
    assert [r["down_k_groups"] for r in rows] == [11, 11, 11, 11, 11, 11, 10, 10]
    assert [r["heads"] for r in rows] == [4] * 8                                  # 32 heads of 128
    # contiguous, complete, head-aligned / group-aligned covers
    for key, total, unit in (("q_cols", 4096, 128), ("kv_cols", 4096, 128), ("down_k_rows", 11008, 128),
                             ("lm_head_cols", 32000, 16)):
        spans = [tuple(r[key]) for r in rows]
        assert spans[0][0] == 0 and spans[-1][1] == total, (key, spans)
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 == b0
        assert all(a % unit == 0 for a, _ in spans), (key, spans)
    for r in rows:
        assert r["o_k_rows"] == r["q_cols"] and r["gate_up_cols"] == r["down_k_rows"]


def test_full_and_dump_outputs_are_options(tmp_path):
    """--full and --dump-outputs DIR parse; a dry run measures nothing and writes nothing."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--full", "--dump-outputs", str(out), "--dry-run"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["world"] == 1
    assert not out.exists()


def test_dump_outputs_writes_float32_npy(tmp_path):
    """dump_outputs writes every array of Runner.outputs() as <name>.npy in float32, whatever dtype the path computes
    in, and tensor-parallel ranks keep their shards apart by name."""
    import numpy as np
    import torch

    import bench

    class FakeRunner:
        def outputs(self):
            return {"o": torch.arange(6, dtype=torch.float16).reshape(2, 3), "logits": torch.ones(1, 5)}

    bench.dump_outputs(FakeRunner(), str(tmp_path / "a"), 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["logits.npy", "o.npy"]
    o = np.load(tmp_path / "a" / "o.npy")
    assert o.dtype == np.float32 and o.shape == (2, 3) and np.array_equal(o.ravel(), np.arange(6, dtype=np.float32))
    bench.dump_outputs(FakeRunner(), str(tmp_path / "b"), 3, 8)
    assert sorted(os.listdir(tmp_path / "b")) == ["logits_rank3.npy", "o_rank3.npy"]


def test_dry_run_single_gpu():
    d = _dry(1)
    assert not d["relaunch"] and d["world"] == 1
    assert d["shards"][0]["down_k_groups"] == 86 and d["shards"][0]["lm_head_cols"] == [0, 32000]
