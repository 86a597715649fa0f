"""Device time of one row gather from a quantized table (DeviceWeight.get_rows: ne_get_rows on the device) next to
torch.index_select on an fp16 copy of a table of the same shape, same session, alternating (development tool).

The method of tools/q6_k_times.py: the calls of a captured graph rotate over copies of the table that together exceed
the 256 MB Infinity Cache, and every call of a graph reads its own set of random ids, so the rows are cold; HIP graph
replay, HIP events on the launch stream.  Each figure is the median of --rounds alternating rounds, with the spread
(min .. max) beside it.  The fp16 table is the comparison the op replaces: a second, unquantized copy of the embedding.

Usage: python tools/get_rows_times.py [--shape 32000x4096] [--ms 1,16,2048] [--rounds 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32000x4096", help="NxK of the table")
    ap.add_argument("--ms", default="1,16,2048")
    ap.add_argument("--reps", type=int, default=32, help="calls per graph")
    ap.add_argument("--replays", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (median reported)")
    ap.add_argument("--mb", type=float, default=400.0, help="MB of rotated table copies (past 256 MB: cold)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from neural_amd import bestla
    n, k = (int(v) for v in args.shape.split("x"))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"{torch.cuda.get_device_name()}  row gather from a {n} x {k} table; us per call (median of {args.rounds} "
        f"alternating rounds, min .. max), cold tables, graph replay")
    say(f"{'table':<12}{'out':>6}{'M':>6}  {'get_rows us':>26}  {'index_select fp16 us':>26}  {'ratio':>6}  "
        f"{'grid':>6}  kernel")
    copies = lambda b: max(2, math.ceil(args.mb * 1e6 / b))  # noqa: E731
    b6 = q6_k_blocks(np, n, k, 6)
    tables = {
        "int4 g128": [bestla.DeviceWeight.synthetic(4, n, k, 128, "fp16", seed=i) for i in range(copies(n * k // 2))],
        "Q6_K": [bestla.DeviceWeight.from_q6_k(b6, n, k) for _ in range(copies(n * k // 256 * 210))],
    }
    dense = [(torch.rand((n, k), device="cuda") - 0.5).to(torch.float16) for _ in range(copies(n * k * 2))]
    for m in (int(v) for v in args.ms.split(",")):
        reps = args.reps if m <= 256 else max(4, args.reps // 4)
        ids = [torch.randint(0, n, (m,), dtype=torch.int32, device="cuda") for _ in range(reps)]
        ids64 = [i.to(torch.int64) for i in ids]
        for oname, odt in (("fp32", torch.float32), ("fp16", torch.float16)):
            out = torch.empty((m, k), dtype=odt, device="cuda")
            out16 = torch.empty((m, k), dtype=torch.float16, device="cuda")
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graphs, times = {}, {}
            with torch.cuda.stream(s):
                def record(key, call):
                    for i in range(reps):  # warm up every copy and the shape
                        call(i)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        for i in range(reps):
                            call(i)
                    g.replay()
                    graphs[key], times[key] = g, []
                for key, wl in tables.items():
                    record(key, lambda i, wl=wl: wl[i % len(wl)].get_rows(ids[i], out=out))
                record("dense", lambda i: torch.index_select(dense[i % len(dense)], 0, ids64[i], out=out16))
                for _ in range(args.rounds):
                    for key in graphs:
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
            for key, wl in tables.items():
                plan = wl[0].plan_get_rows(m, oname)
                say(f"{key:<12}{oname:>6}{m:>6}  {cell[key]:>26}  {cell['dense']:>26}  {med[key] / med['dense']:6.2f}  "
                    f"{plan['grid']:>6}  {plan['kernel']}")
            del graphs
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
