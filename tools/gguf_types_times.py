"""Device time of one forward per GGUF block type (development tool): K x N Q4_1 / Q5_0 / Q5_1 / Q8_0 weights next to
their baselines on the same build -- Q4_0 for Q4_1, a synthetic int8 g32 weight for Q5_0 / Q5_1 / Q8_0 -- at M = 1, 16
and 2048.  Cold weights (rotating copies past the 256 MB Infinity Cache), HIP graph replay, HIP events on the launch
stream, as tools/m_sweep.py.  The min types pay the min-term pass (woq_gguf.hip) on top of the baseline's kernel.

Usage: python tools/gguf_types_times.py [--m 1,16,2048] [--act fp16] [--n 4096] [--k 4096]
"""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BLOCK = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}
NAME = {2: "Q4_0", 3: "Q4_1", 6: "Q5_0", 7: "Q5_1", 8: "Q8_0"}


def random_blocks(np, type, n, k, seed):
    rng = np.random.default_rng(seed)
    nb = k // 32
    b = rng.integers(0, 256, size=(n, nb, BLOCK[type]), dtype=np.uint8)
    b[:, :, 0:2] = rng.uniform(0.001, 0.01, size=(n, nb)).astype(np.float16).view(np.uint8).reshape(n, nb, 2)
    if type in (3, 7):
        b[:, :, 2:4] = rng.uniform(-0.1, 0.1, size=(n, nb)).astype(np.float16).view(np.uint8).reshape(n, nb, 2)
    return b.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,16,2048")
    ap.add_argument("--act", default="fp16")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--mb", type=float, default=400.0, help="MB of rotated weight copies (past 256 MB: cold)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from neural_amd import bestla
    n, k = args.n, args.k
    dt = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[args.act]
    ms = [int(v) for v in args.m.split(",")]
    print(f"{torch.cuda.get_device_name()}  N={n} K={k} act {args.act}; us per forward, cold weights")
    print(f"{'weight':<14}" + "".join(f"{'M=' + str(m):>12}" for m in ms) + "   launches (M=" + ",".join(map(str, ms)) + ")")
    rows = [("Q4_0", 2), ("Q4_1", 3), ("int8 g32", None), ("Q8_0", 8), ("Q5_0", 6), ("Q5_1", 7)]
    for label, type in rows:
        bits = 4 if type in (2, 3) else 8
        copies = max(2, math.ceil(args.mb * 1e6 / (n * k * bits // 8)))
        if type is None:
            ws = [bestla.DeviceWeight.synthetic(8, n, k, 32, "fp16", False, seed=7 + i) for i in range(copies)]
        else:
            blocks = random_blocks(np, type, n, k, type)
            ws = [bestla.DeviceWeight.from_gguf(type, blocks, n, k) for _ in range(copies)]
        line, launches = f"{label:<14}", []
        for m in ms:
            x = (torch.rand((m, k), device="cuda") - 0.5).to(dt)
            out = torch.empty((m, n), device="cuda")
            reps = args.reps if m <= 256 else max(4, args.reps // 4)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for i in range(min(copies, reps)):
                    ws[i % copies].forward(x, out=out)
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=s):
                    for i in range(reps):
                        ws[i % copies].forward(x, out=out)
                gph.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(3):
                    gph.replay()
                e1.record(s)
            torch.cuda.synchronize()
            line += f"{e0.elapsed_time(e1) * 1e3 / (3 * reps):12.2f}"
            launches.append(ws[0].plan(m, args.act)["launches"])
            del gph
        print(line + "   " + ",".join(map(str, launches)), flush=True)
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
