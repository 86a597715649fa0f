"""Device time of the MoE router from the hidden state (development tool): Mixtral-8x7B's ffn_gate_inp, K = 4096, 8
experts, top-2, an fp32 and an fp16 gate, M = 1, 4, 16, 256, 2048 rows.  Two ways, in the same process, alternating, HIP
graph replay, HIP events on the launch stream (the method of tools/moe_times.py):

  (a) nad_moe_gate_route: the gate matmul and the router in one launch;
  (b) what an integrator had before it: torch.matmul(x, gate.T) (hipBLAS) and then nad_moe_route -- with an fp16 gate
      behind the gate's cast to fp32 (gate.float(): one more small launch; the cheaper of the casts that keep the fp32
      activations as they are).  Both write preallocated outputs.

Conditions:
  warm      one gate, a graph of --reps calls on it;
  cold      a graph of one call on every gate of a pool of 512 MiB (4096 fp32 gates, 8192 fp16 gates), twice the 256 MB
            Infinity Cache: no gate is read twice within a replay.  The activations are the same M rows in every call.
  in place  per layer call the router, (a) or (b), and then bestla.moe_ffn on what it wrote, on moe_times.py's walk over
            layers' banks (int4 g128 fp16 scales, cold weights; call j: layer j % L, row r's experts 2 q, 2 q + 1 with
            q = (j // L + r) % 4).  The gate of call j is made so that the router itself picks that walk (checked).
Each figure is the median of --rounds alternating rounds with the spread (min .. max), in us per call.  A way is called
ahead where its whole spread lies below the other's.

Usage: python tools/moe_gate_times.py [--rounds 5] [--replays 100] [--out FILE] [--skip-in-place]
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, NE, TOP_K = 4096, 8, 2
FIN, FMID, FOUT = 4096, 14336, 4096
MS = (1, 4, 16, 256, 2048)
POOL_BYTES = 512 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100, help="graph replays per timed window (warm, in place)")
    ap.add_argument("--reps", type=int, default=16, help="warm: calls per graph")
    ap.add_argument("--cold-replays", type=int, default=2, help="cold: pool walks per timed window")
    ap.add_argument("--skip-in-place", action="store_true")
    ap.add_argument("--out", default=None, help="also write the table here (rewritten after every row)")
    args = ap.parse_args()
    import torch
    from neural_amd import bestla
    from neural_amd._lib import check, lib

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    L_ = lib()
    p = bestla._ptr

    def gate_route(x, gate, ids, wts, s):
        check(L_.nad_moe_gate_route(p(x), x.stride(0), p(gate), bestla._act_code(gate), gate.stride(0), x.shape[0], K, NE,
                                    TOP_K, p(ids), TOP_K, p(wts), TOP_K, None, 0, bestla._stream(s)), "nad_moe_gate_route")

    def matmul_route(x, gate, logits, ids, wts, s):
        g = gate if gate.dtype == torch.float32 else gate.float()
        torch.matmul(x, g.T, out=logits)
        check(L_.nad_moe_route(p(logits), NE, x.shape[0], NE, TOP_K, p(ids), TOP_K, p(wts), TOP_K, bestla._stream(s)),
              "nad_moe_route")

    def measure(fns, calls, replays, warm_calls):
        """fns: key -> fn(j, stream), j the call's index in the graph.  -> key -> [us per call] over the rounds"""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graphs, times = {}, {k: [] for k in fns}
        with torch.cuda.stream(s):
            for key, fn in fns.items():
                for j in range(warm_calls):
                    fn(j, s)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=s):
                    for j in range(calls):
                        fn(j, s)
                gr.replay()
                graphs[key] = gr
            s.synchronize()
            for _ in range(args.rounds):
                for key in fns:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(replays):
                        graphs[key].replay()
                    e1.record(s)
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1) * 1e3 / (replays * calls))
        torch.cuda.synchronize()
        del graphs
        return times

    def cells(times):
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = {k: f"{med[k]:8.2f} ({min(v):.2f} .. {max(v):.2f})" for k, v in times.items()}
        a, b = times["a"], times["b"]
        verdict = "(a) ahead" if max(a) < min(b) else "(b) ahead" if max(b) < min(a) else "spreads overlap"
        return med, cell, verdict

    say(f"{torch.cuda.get_device_name()}  MoE router from the hidden state, K {K}, {NE} experts, top-{TOP_K}, fp32 rows")
    say(f"us per call: median of {args.rounds} alternating rounds (min .. max); (a) nad_moe_gate_route, one launch; (b) "
        f"torch.matmul + nad_moe_route (fp16 gate: gate.float() first)")
    say(f"{'condition':<10}{'gate':>5}{'M':>6}{'calls':>6}  {'(a) us':>26}  {'(b) us':>26}  {'a/b':>5}  verdict")
    for dtype, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
        gen = torch.Generator(device="cuda").manual_seed(7)
        gbytes = NE * K * (4 if dtype == torch.float32 else 2)
        pool_n = POOL_BYTES // gbytes
        pool = ((torch.rand((pool_n, NE, K), device="cuda", generator=gen) - 0.5) / 8).to(dtype)
        for m in MS:
            x = torch.rand((m, K), device="cuda", generator=gen) - 0.5
            ids = {k: torch.empty((m, TOP_K), dtype=torch.int32, device="cuda") for k in "ab"}
            wts = {k: torch.empty((m, TOP_K), device="cuda") for k in "ab"}
            logits = torch.empty((m, NE), device="cuda")
            for cond, calls, replays, gate_of in (("warm", args.reps, args.replays, lambda j: pool[0]),
                                                  ("cold", pool_n, args.cold_replays, lambda j: pool[j])):
                fns = {"a": lambda j, s: gate_route(x, gate_of(j), ids["a"], wts["a"], s),
                       "b": lambda j, s: matmul_route(x, gate_of(j), logits, ids["b"], wts["b"], s)}
                times = measure(fns, calls, replays, min(calls, 4))
                # the last call of both graphs ran the same gate on the same rows
                same = bool(torch.equal(ids["a"], ids["b"]))
                dw = float((wts["a"] - wts["b"]).abs().max())
                med, cell, verdict = cells(times)
                say(f"{cond:<10}{name:>5}{m:>6}{calls:>6}  {cell['a']:>26}  {cell['b']:>26}  {med['a'] / med['b']:5.2f}  "
                    f"{verdict}{'' if same else '  [ids differ between (a) and (b)]'}  max |wts a - b| {dw:.1e}")
        del pool
        torch.cuda.empty_cache()

    if not args.skip_in_place:
        say("")
        say(f"in place: the router and bestla.moe_ffn per layer call, Mixtral-8x7B FFN layer fin {FIN} fmid {FMID} fout "
            f"{FOUT}, int4 g128 f16, cold weights; us per layer call")
        say(f"{'gate':>5}{'M':>4}{'L':>3}{'reps':>5}  {'(a) gate_route + moe_ffn us':>30}  {'(b) matmul + route + moe_ffn us':>32}  "
            f"{'a/b':>5}  {'(a) us/token-layer':>18}  {'(b) us/token-layer':>18}  verdict")

        def make(n, k, seed):
            return bestla.DeviceWeight.synthetic(4, n, k, 128, "fp16", False, seed=seed)

        probe = [make(FMID, FIN, 1), make(FMID, FIN, 2), make(FOUT, FMID, 3)]
        expert_bytes = sum(w.bytes for w in probe)
        del probe
        L = max(2, math.ceil(2 ** 30 / (NE * expert_bytes)))
        layers = []
        for li in range(L):
            g = [make(FMID, FIN, 1000 * li + e) for e in range(NE)]
            u = [make(FMID, FIN, 1000 * li + 100 + e) for e in range(NE)]
            d = [make(FOUT, FMID, 1000 * li + 200 + e) for e in range(NE)]
            layers.append((bestla.ExpertBank(g), bestla.ExpertBank(u), bestla.ExpertBank(d), g, u, d))
        reps = L * 4
        for dtype, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
            for m in (1, 4):
                x = torch.rand((m, FIN), device="cuda") - 0.5
                want = [[[2 * ((j // L + r) % 4) + i for i in range(TOP_K)] for r in range(m)] for j in range(reps)]
                # gate_j with x . gate_j^T = C_j: logit 2 for the row's first expert, 1 for its second, 0 elsewhere
                pinv = torch.linalg.pinv(x.double().cpu())  # [K][m]
                gates = []
                for j in range(reps):
                    c = torch.zeros((m, NE), dtype=torch.float64)
                    for r in range(m):
                        c[r, want[j][r][0]], c[r, want[j][r][1]] = 2.0, 1.0
                    gates.append((pinv @ c).T.contiguous().to(dtype).cuda())
                ids = {k: torch.empty((m, TOP_K), dtype=torch.int32, device="cuda") for k in "ab"}
                wts = {k: torch.empty((m, TOP_K), device="cuda") for k in "ab"}
                out = {k: torch.empty((m, FOUT), device="cuda") for k in "ab"}
                ws = {k: bestla.moe_workspace_alloc(m, TOP_K, FMID, FOUT) for k in "ab"}
                logits = torch.empty((m, NE), device="cuda")
                for j in range(reps):  # the router picks the walk
                    gate_route(x, gates[j], ids["a"], wts["a"], None)
                    assert ids["a"].cpu().tolist() == want[j], (j, ids["a"].cpu().tolist(), want[j])

                def ffn(key, j, s):
                    gb, ub, db = layers[j % L][:3]
                    bestla.moe_ffn(gb, ub, db, x, ids[key], wts[key], out=out[key], stream=s, workspace=ws[key])

                def run_a(j, s):
                    gate_route(x, gates[j], ids["a"], wts["a"], s)
                    ffn("a", j, s)

                def run_b(j, s):
                    matmul_route(x, gates[j], logits, ids["b"], wts["b"], s)
                    ffn("b", j, s)

                times = measure({"a": run_a, "b": run_b}, reps, args.replays, reps)
                assert torch.equal(ids["a"], ids["b"])
                diff = float((out["a"] - out["b"]).abs().max() / out["a"].abs().max())
                med, cell, verdict = cells(times)
                say(f"{name:>5}{m:>4}{L:>3}{reps:>5}  {cell['a']:>30}  {cell['b']:>32}  {med['a'] / med['b']:5.2f}  "
                    f"{med['a'] / m:18.2f}  {med['b'] / m:18.2f}  {verdict}  out a-b rel diff {diff:.1e}")
        del layers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
