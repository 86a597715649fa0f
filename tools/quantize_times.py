"""Load-time quantization of an fp16 checkpoint matrix that already sits in HBM: the device entry (nad_device_quantize
through DeviceWeight.quantize: three kernels of woq_quant.hip, the repack, a copy-back of the scale buffer) next to the
host path on the same matrix and the same box -- the copy down and the widening to fp32, BTLAGemmQuantPackB on
--threads host threads, nad_device_load (development tool).

Both entries are synchronous, so each figure is a host clock around a call that ends in a device synchronise: the
median of --rounds calls (after one warm-up call) with the spread (min .. max) beside it.  The byte time is what the
entry must move at least -- the input matrix once and the device layout once -- at 8 TB/s; the kernels' own share of
the entry's time comes from a kernel trace of this tool (--no-host keeps the trace to the device entry).

Usage: python tools/quantize_times.py [--shapes 4096x4096;11008x4096;4096x11008;32000x4096] [--group 128]
           [--weight int4] [--scale fp16] [--act fp16] [--rounds 7] [--host-rounds 3] [--threads 16] [--no-host]

--host-load times the two host load entries alone, per shape: nad_device_load of the packed blob and
nad_gguf_device_load of a Q4_1 matrix of the same shape (stage, repack, synchronise, free; --rounds calls each).  To
compare two builds, run it once per build with NAD_LIB_PATH, alternating, and read the difference against the spread
the same build shows between its own runs.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, rounds, sync):
    fn()
    sync()
    out = []
    for _ in range(rounds):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def cell(v):
    return f"{statistics.median(v):10.3f} ({min(v):.3f} .. {max(v):.3f})"


def host_load(args, np, bestla, sync):
    print(f"library {os.path.basename(bestla.lib()._name)}; ms per call, median (min .. max) of {args.rounds} calls")
    print(f"{'N x K':<14}{'nad_device_load ms':>34}{'nad_gguf_device_load Q4_1 ms':>36}")
    for shape in args.shapes.split(";"):
        n, k = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(n + k)
        blob = bestla.quantize(rng.standard_normal((n, k), dtype=np.float32), group_size=args.group,
                               weight_dtype=args.weight, scale_dtype=args.scale)
        blocks = rng.integers(0, 256, size=(n * (k // 32), 20), dtype=np.uint8)  # block_q4_1: fp16 d, fp16 m, 16 bytes
        blocks[:, 0:4] = rng.uniform(1e-3, 1e-2, (n * (k // 32), 2)).astype(np.float16).view(np.uint8)
        t_blob = timed(lambda: bestla.DeviceWeight(blob), args.rounds, sync)
        t_gguf = timed(lambda: bestla.DeviceWeight.from_gguf(bestla.GGUF_Q4_1, blocks, n, k), args.rounds, sync)
        print(f"{shape:<14}{cell(t_blob):>34}{cell(t_gguf):>36}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096;11008x4096;4096x11008;32000x4096", help="NxK;NxK;...")
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--weight", default="int4")
    ap.add_argument("--scale", default="fp16")
    ap.add_argument("--act", default="fp16", help="dtype of the matrix in HBM")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-load", action="store_true", help="time nad_device_load and nad_gguf_device_load (Q4_1) only")
    args = ap.parse_args()
    os.environ["NAD_HOST_THREADS"] = str(args.threads)
    import numpy as np
    import torch
    from neural_amd import bestla
    dt = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[args.act]
    esz = 4 if args.act == "fp32" else 2
    kw = dict(group_size=args.group, weight_dtype=args.weight, scale_dtype=args.scale)
    sync = torch.cuda.synchronize
    if args.host_load:
        return host_load(args, np, bestla, sync)
    print(f"{torch.cuda.get_device_name()}  {args.weight} g{args.group}, {args.scale} scales, {args.act} input; ms per "
          f"call, median (min .. max) of {args.rounds} device / {args.host_rounds} host calls; host path on "
          f"{args.threads} threads")
    print(f"{'N x K':<14}{'device entry ms':>34}{'byte time ms':>14}{'entry/byte':>12}"
          f"{'host: copy + widen ms':>34}{'BTLAGemmQuantPackB ms':>36}{'nad_device_load ms':>34}{'host/device':>12}")
    for shape in args.shapes.split(";"):
        n, k = (int(v) for v in shape.split("x"))
        torch.manual_seed(n + k)
        w = torch.randn((n, k), device="cuda").to(dt)
        dev = timed(lambda: bestla.DeviceWeight.quantize(w, **kw), args.rounds, sync)
        dw = bestla.DeviceWeight.quantize(w, **kw)
        byte_ms = (n * k * esz + dw.bytes) / 8e12 * 1e3
        line = f"{shape:<14}{cell(dev):>34}{byte_ms:14.4f}{statistics.median(dev) / byte_ms:12.1f}"
        if not args.no_host:
            state = {}

            def down():
                state["w32"] = w.cpu().numpy().astype(np.float32)

            def pack():
                state["blob"] = bestla.quantize(state["w32"], **kw)

            def load():
                state["dw"] = bestla.DeviceWeight(state["blob"])

            t_down = timed(down, args.host_rounds, sync)
            t_pack = timed(pack, args.host_rounds, sync)
            t_load = timed(load, args.host_rounds, sync)
            host = statistics.median(t_down) + statistics.median(t_pack) + statistics.median(t_load)
            same = torch.equal(state["dw"].mem[:dw.bytes].view(torch.uint8)[:256], dw.mem[:256])
            line += (f"{cell(t_down):>34}{cell(t_pack):>36}{cell(t_load):>34}{host / statistics.median(dev):12.1f}"
                     f"{'' if same else '  (layouts differ!)'}")
        print(line, flush=True)
        del w, dw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
