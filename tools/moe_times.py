"""Device time of one routed Mixtral-8x7B FFN layer at decode sizes (development tool): fin = fout = 4096, fmid = 14336,
8 experts, top-2, M = 1 and M = 4 rows, in two formats -- int4 g128 fp16 scales, and the int2 policy (int2 g64 gate / up,
int4 g128 down; llama_utils.cpp:269-287).  Two ways, in the same process, alternating, HIP graph replay, HIP events on
the launch stream:

  (a) bestla.moe_ffn: the routing read on the device, three launches per layer call;
  (b) what the library could do before it, given the ids on the host already: per (row, slot) one bestla.ffn_forward at
      M = 1 on that expert's three weights, then torch mul / addcmul for the weighted sum.  This is generous to (b): in
      real use it also copies the ids to the host and synchronises, in every layer, and cannot be captured at all.

Cold weights: a graph holds `reps` layer calls that walk over L layers' banks and, within a layer, over its experts
(call j: layer j % L, row r's experts 2 q, 2 q + 1 with q = (j // L + r) % 4), L chosen so that the banks together exceed
1 GiB: no weight is read twice within a replay, and a replay streams several times the 256 MB Infinity Cache between two
reads of the same weight.  Each figure is the median of --rounds alternating rounds with the spread (min .. max).
Bytes: per (row, slot) the three weights' device bytes (tiles + scales), the activation row and the output row, over
the time, as a fraction of 8 TB/s.

Usage: python tools/moe_times.py [--rounds 5] [--replays 200] [--out FILE]

--grouped: the same layer at batched-decode and prefill sizes (M = 8, 16, 64, 256, 2048; a random top-2 routing, experts
distinct per row), three ways, alternating in one process, graph replay, HIP events:

  (a) bestla.moe_ffn_grouped: sorted on the device, grouped gemm7, six launches;
  (b) bestla.moe_ffn: the row-routed form, every problem streaming its expert's weights (few replays where M is large);
  (c) what the library could do without either, given the ids on the host already: the rows gathered into expert order
      (index_select), one bestla.ffn_forward per expert on its contiguous rows, and the weighted sum over the slots
      (index_select, multiply, sum).  As above this leaves out the ids' copy to the host and the synchronisation.

A graph holds one call on each of two layers' banks (one layer's experts are 0.7 GB int4: more than the Infinity Cache
on their own).  A window replays the graph until it has run about --window-ms.

--general: the formats only a general bank takes (ExpertBank(..., general=True): woq_gemv_routed_kernel, and the grouped
gemm7's groups of 32 / int8) instead of the two above -- int4 g32 with fp32 scales (the reference's default
quantization), and the layouts GGUF Q4_0 (int4 g32, fp16 scales) and Q8_0 (int8 g32, fp16 scales) load into.  The
per-expert ffn_forward calls are then the only way the library could run these banks before; with --grouped, M = 64,
256 and 2048.

--q6k: the layer with every weight GGUF Q6_K (the published model.Q6_K.gguf of Mixtral; a general bank of route kind 2:
woq_q6k_gemv_routed_kernel, four launches per layer call, and with --grouped woq_q6k_gemm_grouped_kernel at M = 16, 64,
256 and 2048).  The blocks are random bytes with d in 5e-6 .. 2e-5 (weights of about 1 / sqrt(K), so that the FFN's
intermediate stays inside the fp16 range of its hi part), one array per shape loaded into every expert's own device
memory.  (b) / (c) are again the per-expert ffn_forward calls with the ids on the host.
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIN, FMID, FOUT, NE, TOP_K = 4096, 14336, 4096, 8, 2
PEAK = 8e12
FORMATS = {  # (bits, group, scale type) of gate / up, of down
    "int4 g128 f16": ((4, 128, "fp16"), (4, 128, "fp16")),
    "int2 g64 gate/up + int4 g128 down": ((2, 64, "fp16"), (4, 128, "fp16")),
}
Q6K_FORMATS = {"Q6_K": ((6, 16, "fp16"), (6, 16, "fp16"))}
GENERAL_FORMATS = {
    "int4 g32 f32 (reference default)": ((4, 32, "fp32"), (4, 32, "fp32")),
    "Q4_0 layout (int4 g32 f16)": ((4, 32, "fp16"), (4, 32, "fp16")),
    "Q8_0 layout (int8 g32 f16)": ((8, 32, "fp16"), (8, 32, "fp16")),
}


def formats(args):
    return Q6K_FORMATS if args.q6k else (GENERAL_FORMATS if args.general else FORMATS)


_Q6K_BLOCKS = {}


def make_weight(bestla, bits, n, k, gs, st, seed):
    """a synthetic weight of the format; bits 6: Q6_K from random block bytes (made once per shape) with a finite d"""
    if bits != 6:
        return bestla.DeviceWeight.synthetic(bits, n, k, gs, st, False, seed=seed)
    import numpy as np
    if (n, k) not in _Q6K_BLOCKS:
        rng = np.random.default_rng(n + k)
        b = rng.integers(0, 256, size=(n, k // 256, 210), dtype=np.uint8)
        d = rng.uniform(5e-6, 2e-5, size=(n, k // 256)).astype(np.float16)  # weights of about 1 / sqrt(K): finite t
        b[:, :, 208:210] = d.reshape(n, k // 256, 1).view(np.uint8)
        _Q6K_BLOCKS[(n, k)] = b.ravel()
    return bestla.DeviceWeight.from_q6_k(_Q6K_BLOCKS[(n, k)], n, k)


def grouped(args):
    import torch
    from neural_amd import bestla

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}  Mixtral-8x7B FFN layer, fin {FIN} fmid {FMID} fout {FOUT}, {NE} experts, "
        f"top-{TOP_K}, fp32 rows, random routing")
    say(f"us per layer call: median of {args.rounds} alternating rounds (min .. max); a graph of 2 layer calls replayed "
        f"for about {args.window_ms} ms per window")
    say(f"{'format':<36}{'M':>5} {'bm':>4}  {'(a) moe_ffn_grouped us':>30}  {'(b) moe_ffn us':>32}  "
        f"{'(c) per-expert ffn_forward us':>32}  {'a/b':>6}  {'a/c':>6}  {'(a) TFLOP/s':>11}  {'a-b diff':>9}  {'a-c diff':>9}")
    L = 2
    for name, ((gbits, ggs, gst), (dbits, dgs, dst)) in formats(args).items():
        def make(bits, n, k, gs, st, seed):
            return make_weight(bestla, bits, n, k, gs, st, seed)

        def bank(ws):
            return bestla.ExpertBank(ws, general=args.general or args.q6k)

        layers = []
        for li in range(L):
            g = [make(gbits, FMID, FIN, ggs, gst, 1000 * li + e) for e in range(NE)]
            u = [make(gbits, FMID, FIN, ggs, gst, 1000 * li + 100 + e) for e in range(NE)]
            d = [make(dbits, FOUT, FMID, dgs, dst, 1000 * li + 200 + e) for e in range(NE)]
            layers.append((g, u, d, bank(g), bank(u), bank(d)))
        for m in ((16, 64, 256, 2048) if args.q6k else (64, 256, 2048) if args.general else (8, 16, 64, 256, 2048)):
            np_ = m * TOP_K
            gen = torch.Generator(device="cuda").manual_seed(m)
            x = torch.rand((m, FIN), device="cuda", generator=gen) - 0.5
            ids = torch.rand((m, NE), device="cuda", generator=gen).topk(TOP_K, dim=1).indices.to(torch.int32)
            w = torch.rand((m, TOP_K), device="cuda", generator=gen) + 0.1
            w = (w / w.sum(dim=1, keepdim=True)).contiguous()
            # (c)'s host-side routing, made once outside the timed region
            flat = ids.flatten().cpu()
            order = torch.sort(flat, stable=True).indices
            counts = torch.bincount(flat, minlength=NE).tolist()
            src = (order // TOP_K).cuda()
            inv = torch.empty(np_, dtype=torch.int64)
            inv[order] = torch.arange(np_)
            inv = inv.cuda()
            outs = {k: torch.empty((m, FOUT), device="cuda") for k in "abc"}
            xs = torch.empty((np_, FIN), device="cuda")
            ys = torch.empty((np_, FOUT), device="cuda")
            yp = torch.empty((np_, FOUT), device="cuda")
            tmp1 = torch.empty((np_, FMID), device="cuda")
            tmp2 = torch.empty((np_, FMID), device="cuda")
            gb0, ub0, db0 = layers[0][3:]
            ws_a = bestla.moe_grouped_workspace_alloc(gb0, ub0, db0, m, TOP_K)
            ws_b = bestla.moe_workspace_alloc(m, TOP_K, FMID, FOUT)

            def run_a(j, s):
                _, _, _, gb, ub, db = layers[j]
                bestla.moe_ffn_grouped(gb, ub, db, x, ids, w, out=outs["a"], stream=s, workspace=ws_a)

            def run_b(j, s):
                _, _, _, gb, ub, db = layers[j]
                bestla.moe_ffn(gb, ub, db, x, ids, w, out=outs["b"], stream=s, workspace=ws_b)

            def run_c(j, s):
                g, u, d, _, _, _ = layers[j]
                torch.index_select(x, 0, src, out=xs)
                o = 0
                for e in range(NE):
                    c = counts[e]
                    if c:
                        bestla.ffn_forward(xs[o:o + c], g[e], d[e], u[e], tmp1=tmp1[o:o + c], tmp2=tmp2[o:o + c],
                                           out=ys[o:o + c], stream=s)
                    o += c
                torch.index_select(ys, 0, inv, out=yp)
                torch.sum(yp.view(m, TOP_K, FOUT) * w[:, :, None], dim=1, out=outs["c"])

            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graphs, replays, times = {}, {}, {k: [] for k in "abc"}
            with torch.cuda.stream(s):
                for key, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
                    for j in range(L):
                        fn(j, s)
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=s):
                        for j in range(L):
                            fn(j, s)
                    gr.replay()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    gr.replay()
                    e1.record(s)
                    e1.synchronize()
                    graphs[key] = gr
                    replays[key] = max(1, min(args.replays, int(args.window_ms / max(e0.elapsed_time(e1), 1e-3))))
                s.synchronize()
                scale = float(outs["a"].abs().max())
                dab = float((outs["a"] - outs["b"]).abs().max()) / scale
                dac = float((outs["a"] - outs["c"]).abs().max()) / scale
                for _ in range(args.rounds):
                    for key in "abc":
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(replays[key]):
                            graphs[key].replay()
                        e1.record(s)
                        e1.synchronize()
                        times[key].append(e0.elapsed_time(e1) * 1e3 / (replays[key] * L))
            torch.cuda.synchronize()
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = {k: f"{med[k]:10.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times.items()}
            bm = bestla.plan_moe_grouped(gb0, ub0, db0, m, TOP_K)["bm"]
            flops = 2.0 * np_ * (2 * FIN * FMID + FMID * FOUT)
            say(f"{name:<36}{m:>5} {bm:>4}  {cell['a']:>30}  {cell['b']:>32}  {cell['c']:>32}  "
                f"{med['a'] / med['b']:6.3f}  {med['a'] / med['c']:6.3f}  {flops / med['a'] * 1e-6:11.1f}  {dab:9.1e}  "
                f"{dac:9.1e}")
            del graphs
        plan = bestla.plan_moe_grouped(layers[0][3], layers[0][4], layers[0][5], 2048, TOP_K)
        say("  launches at M = 2048: " + ", ".join(f"{p['kernel']} grid {p['grid']} x {p['threads']}"
                                                   for p in plan["launches"]) +
            f"; tile height {plan['bm']}, tile bound {plan['bound']}")
        del layers
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grouped", action="store_true", help="M = 16 .. 2048: grouped vs row-routed vs per-expert calls")
    ap.add_argument("--general", action="store_true", help="the formats of general banks: int4 g32 f32, Q4_0, Q8_0")
    ap.add_argument("--q6k", action="store_true", help="every weight GGUF Q6_K (a general bank of route kind 2)")
    ap.add_argument("--window-ms", type=float, default=60.0, help="--grouped: about this much work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200, help="graph replays per timed window")
    ap.add_argument("--gib", type=float, default=1.0, help="distinct weight bytes a replay streams, at least")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if args.grouped:
        return grouped(args)
    import torch
    from neural_amd import bestla

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}  Mixtral-8x7B FFN layer, fin {FIN} fmid {FMID} fout {FOUT}, {NE} experts, "
        f"top-{TOP_K}, fp32 rows")
    say(f"us per layer call: median of {args.rounds} alternating rounds (min .. max), {args.replays} graph replays per "
        f"window, cold weights")
    say(f"{'format':<36}{'M':>3} {'L':>2} {'reps':>4}  {'(a) moe_ffn us':>28}  {'(b) per-expert ffn_forward us':>30}  "
        f"{'a/b':>5}  {'(a) us/token-layer':>18}  {'(a) of 8 TB/s':>13}  {'(b) of 8 TB/s':>13}")
    for name, ((gbits, ggs, gst), (dbits, dgs, dst)) in formats(args).items():
        def make(bits, n, k, gs, st, seed):
            return make_weight(bestla, bits, n, k, gs, st, seed)

        def bank(ws):
            return bestla.ExpertBank(ws, general=args.general or args.q6k)

        probe = [make(gbits, FMID, FIN, ggs, gst, 1), make(gbits, FMID, FIN, ggs, gst, 2),
                 make(dbits, FOUT, FMID, dgs, dst, 3)]
        expert_bytes = sum(w.bytes for w in probe)
        del probe
        L = max(2, math.ceil(args.gib * 2 ** 30 / (NE * expert_bytes)))
        layers = []
        for li in range(L):
            g = [make(gbits, FMID, FIN, ggs, gst, 1000 * li + e) for e in range(NE)]
            u = [make(gbits, FMID, FIN, ggs, gst, 1000 * li + 100 + e) for e in range(NE)]
            d = [make(dbits, FOUT, FMID, dgs, dst, 1000 * li + 200 + e) for e in range(NE)]
            layers.append((g, u, d, bank(g), bank(u), bank(d)))
        reps = L * 4
        for m in (1, 4):
            x = torch.rand((m, FIN), device="cuda") - 0.5
            w = torch.rand((m, TOP_K), device="cuda") + 0.1
            w = w / w.sum(dim=1, keepdim=True)
            out_a = torch.empty((m, FOUT), device="cuda")
            out_b = torch.empty((m, FOUT), device="cuda")
            tmp1 = torch.empty((1, FMID), device="cuda")
            tmp2 = torch.empty((1, FMID), device="cuda")
            ys = [torch.empty((1, FOUT), device="cuda") for _ in range(TOP_K)]
            ids_h = [[[2 * ((j // L + r) % 4) + i for i in range(TOP_K)] for r in range(m)] for j in range(reps)]
            ids_d = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in ids_h]

            def run_a(j, s):
                _, _, _, gb, ub, db = layers[j % L]
                bestla.moe_ffn(gb, ub, db, x, ids_d[j], w, out=out_a, stream=s)

            def run_b(j, s):
                g, u, d, _, _, _ = layers[j % L]
                for r in range(m):
                    for i in range(TOP_K):
                        e = ids_h[j][r][i]
                        bestla.ffn_forward(x[r:r + 1], g[e], d[e], u[e], tmp1=tmp1, tmp2=tmp2, out=ys[i], stream=s)
                    torch.mul(ys[0], w[r:r + 1, 0:1], out=out_b[r:r + 1])
                    for i in range(1, TOP_K):
                        torch.addcmul(out_b[r:r + 1], ys[i], w[r:r + 1, i:i + 1], out=out_b[r:r + 1])

            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graphs, times = {}, {"a": [], "b": []}
            with torch.cuda.stream(s):
                for key, fn in (("a", run_a), ("b", run_b)):
                    for j in range(reps):  # warm up every bank and the shape
                        fn(j, s)
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=s):
                        for j in range(reps):
                            fn(j, s)
                    gr.replay()
                    graphs[key] = gr
                s.synchronize()
                # the two ways compute the same layer (the last call's rows; (b) fuses its multiply-adds)
                diff = float((out_a - out_b).abs().max() / out_a.abs().max())
                assert diff < 1e-5, diff
                for _ in range(args.rounds):
                    for key in ("a", "b"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(args.replays):
                            graphs[key].replay()
                        e1.record(s)
                        e1.synchronize()
                        times[key].append(e0.elapsed_time(e1) * 1e3 / (args.replays * reps))
            torch.cuda.synchronize()
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = {k: f"{med[k]:9.2f} ({min(v):.2f} .. {max(v):.2f})" for k, v in times.items()}
            nbytes = m * TOP_K * (expert_bytes + FIN * 4 + FOUT * 4)
            frac = {k: nbytes / (med[k] * 1e-6) / PEAK for k in med}
            say(f"{name:<36}{m:>3} {L:>2} {reps:>4}  {cell['a']:>28}  {cell['b']:>30}  {med['a'] / med['b']:5.2f}  "
                f"{med['a'] / m:18.2f}  {frac['a']:13.2f}  {frac['b']:13.2f}")
            del graphs
        plan = bestla.plan_moe(layers[0][3], layers[0][4], layers[0][5], 1, TOP_K)
        say(f"  launches at M = 1: " + ", ".join(f"{p['kernel']} grid {p['grid']} x {p['threads']}" for p in plan))
        del layers
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
