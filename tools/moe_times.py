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
FORMATS = {
    "int4 g128 f16": ((4, 128), (4, 128)),
    "int2 g64 gate/up + int4 g128 down": ((2, 64), (4, 128)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200, help="graph replays per timed window")
    ap.add_argument("--gib", type=float, default=1.0, help="distinct weight bytes a replay streams, at least")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
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
    for name, ((gbits, ggs), (dbits, dgs)) in FORMATS.items():
        def make(bits, n, k, gs, seed):
            return bestla.DeviceWeight.synthetic(bits, n, k, gs, "fp16", False, seed=seed)

        probe = [make(gbits, FMID, FIN, ggs, 1), make(gbits, FMID, FIN, ggs, 2), make(dbits, FOUT, FMID, dgs, 3)]
        expert_bytes = sum(w.bytes for w in probe)
        del probe
        L = max(2, math.ceil(args.gib * 2 ** 30 / (NE * expert_bytes)))
        layers = []
        for li in range(L):
            g = [make(gbits, FMID, FIN, ggs, 1000 * li + e) for e in range(NE)]
            u = [make(gbits, FMID, FIN, ggs, 1000 * li + 100 + e) for e in range(NE)]
            d = [make(dbits, FOUT, FMID, dgs, 1000 * li + 200 + e) for e in range(NE)]
            layers.append((g, u, d, bestla.ExpertBank(g), bestla.ExpertBank(u), bestla.ExpertBank(d)))
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
