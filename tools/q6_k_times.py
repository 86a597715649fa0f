"""Device time of one GGUF Q6_K forward -- in fp (the default) and in the weight's COMPUTE_Q8_K mode (woq_q6k_i8_kernel:
Q8_K activation rows, integer dot products) -- next to Q8_0 (the int8 g32 path: what a Q6_K tensor had to be
requantized to before this layout existed), same shapes, same run, alternating (development tool).  Cold weights: the forwards of a
captured graph rotate over copies of the weight that together exceed the 256 MB Infinity Cache; HIP graph replay, HIP
events on the launch stream (the method of tools/gguf_types_times.py).  Each figure is the median of --rounds
alternating rounds, with the spread (min .. max) beside it.  For M = 1 the achieved bandwidth is the algorithmic bytes
-- the file's weight bytes (210 per 256 weights for Q6_K, 34 per 32 for Q8_0), the activation row and the fp32 output
row -- over that time.

Usage: python tools/q6_k_times.py [--shapes 4096x4096:1,16,2048;32000x4096:1] [--act fp16] [--rounds 5]
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def q6_k_blocks(np, n, k, seed):
    rng = np.random.default_rng(seed)
    nb = k // 256
    b = rng.integers(0, 256, size=(n, nb, 210), dtype=np.uint8)
    b[:, :, 208:210] = rng.uniform(1e-4, 1e-2, size=(n, nb)).astype(np.float16).view(np.uint8).reshape(n, nb, 2)
    return b.ravel()


def q8_0_blocks(np, n, k, seed):
    rng = np.random.default_rng(seed)
    nb = k // 32
    b = rng.integers(0, 256, size=(n, nb, 34), dtype=np.uint8)
    b[:, :, 0:2] = rng.uniform(0.001, 0.01, size=(n, nb)).astype(np.float16).view(np.uint8).reshape(n, nb, 2)
    return b.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096:1,16,2048;32000x4096:1", help="NxK:M,M,...;...")
    ap.add_argument("--act", default="fp16")
    ap.add_argument("--reps", type=int, default=32, help="forwards per graph")
    ap.add_argument("--replays", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (median reported)")
    ap.add_argument("--mb", type=float, default=400.0, help="MB of rotated weight copies (past 256 MB: cold)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from neural_amd import bestla
    dt = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[args.act]
    esz = 4 if args.act == "fp32" else 2
    print(f"{torch.cuda.get_device_name()}  act {args.act}; us per forward (median of {args.rounds} alternating rounds, "
          f"min .. max), cold weights")
    print(f"{'N x K':<14}{'M':>6}  {'Q6_K us':>26}  {'Q6_K in Q8_K mode us':>26}  {'Q8_0 us':>26}  {'Q6_K/Q8_0':>9}  "
          f"{'mode/fp':>7}  {'Q6_K TB/s':>9}  {'mode TB/s':>9}  {'Q8_0 TB/s':>9}  kernels")
    for spec in args.shapes.split(";"):
        shape, ms = spec.split(":")
        n, k = (int(v) for v in shape.split("x"))
        wbytes = {"q6": n * k // 256 * 210, "q6i": n * k // 256 * 210, "q8": n * k // 32 * 34}
        b6, b8 = q6_k_blocks(np, n, k, 6), q8_0_blocks(np, n, k, 8)
        ws = {"q6": [bestla.DeviceWeight.from_q6_k(b6, n, k)
                     for _ in range(max(2, math.ceil(args.mb * 1e6 / wbytes["q6"])))],
              "q6i": [bestla.DeviceWeight.from_q6_k(b6, n, k).set_compute(bestla.COMPUTE_Q8_K)
                      for _ in range(max(2, math.ceil(args.mb * 1e6 / wbytes["q6i"])))],
              "q8": [bestla.DeviceWeight.from_gguf(bestla.GGUF_Q8_0, b8, n, k)
                     for _ in range(max(2, math.ceil(args.mb * 1e6 / wbytes["q8"])))]}
        for m in (int(v) for v in ms.split(",")):
            x = (torch.rand((m, k), device="cuda") - 0.5).to(dt)
            out = torch.empty((m, n), device="cuda")
            reps = args.reps if m <= 256 else max(4, args.reps // 4)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graphs, times = {}, {"q6": [], "q6i": [], "q8": []}
            with torch.cuda.stream(s):
                for key, wl in ws.items():
                    for i in range(max(len(wl), 2)):  # warm up every weight copy and the shape
                        wl[i % len(wl)].forward(x, out=out)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        for i in range(reps):
                            wl[i % len(wl)].forward(x, out=out)
                    g.replay()
                    graphs[key] = g
                for _ in range(args.rounds):
                    for key in ("q6", "q6i", "q8"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(args.replays):
                            graphs[key].replay()
                        e1.record(s)
                        e1.synchronize()
                        times[key].append(e0.elapsed_time(e1) * 1e3 / (args.replays * reps))
            torch.cuda.synchronize()
            med = {key: statistics.median(v) for key, v in times.items()}
            cell = {key: f"{med[key]:9.2f} ({min(v):.2f} .. {max(v):.2f})" for key, v in times.items()}
            tbs = {key: (wbytes[key] + k * esz + n * 4) / (med[key] * 1e-6) / 1e12 for key in med}
            bw = (f"{tbs['q6']:9.2f}  {tbs['q6i']:9.2f}  {tbs['q8']:9.2f}" if m == 1
                  else f"{'':>9}  {'':>9}  {'':>9}")
            kern = " / ".join(ws[key][0].plan(m, args.act)["kernel"] for key in ("q6", "q6i", "q8"))
            print(f"{shape:<14}{m:>6}  {cell['q6']:>26}  {cell['q6i']:>26}  {cell['q8']:>26}  "
                  f"{med['q6'] / med['q8']:9.2f}  {med['q6i'] / med['q6']:7.2f}  {bw}  {kern}", flush=True)
            del graphs
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
