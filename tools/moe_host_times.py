"""Host cost of one eager routed-FFN call (development tool): wall time per call of bestla.moe_ffn at M = 1 and of
bestla.moe_ffn_grouped at M = 16 on the small test shapes (fin 1024, fmid 512, fout 300, 4 experts, top-2, int4 g128),
where the launches are short and the host side of the entry shows.  CALLS calls after WARM warm-up calls, one stream
synchronisation at the end; us_enqueue is the same window up to the last call's return.  Prints one JSON line.

A/B of two builds: alternate them, one process each, over a few rounds and compare the medians against the first
build's own round-to-round spread:

  for r in 1 2 3 4 5; do for l in OLD.so NEW.so; do NAD_LIB_PATH=$l python tools/moe_host_times.py; done; done
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIN, FMID, FOUT, NE, TOP_K = 1024, 512, 300, 4, 2
CALLS, WARM = 4000, 500


def main():
    import torch
    from neural_amd import bestla

    def bank(n, k, seed):
        return bestla.ExpertBank([bestla.DeviceWeight.synthetic(4, n, k, 128, "fp16", False, seed=seed + e)
                                  for e in range(NE)])

    gate, up, down = bank(FMID, FIN, 0), bank(FMID, FIN, 100), bank(FOUT, FMID, 200)
    s = torch.cuda.Stream()
    res = {"lib": os.environ.get("NAD_LIB_PATH", "libneural_amd.so")}
    with torch.cuda.stream(s):
        for name, m, grouped in (("moe_ffn M=1", 1, False), ("moe_ffn_grouped M=16", 16, True)):
            gen = torch.Generator(device="cuda").manual_seed(m)
            x = torch.rand((m, FIN), device="cuda", generator=gen) - 0.5
            ids = torch.rand((m, NE), device="cuda", generator=gen).topk(TOP_K, dim=1).indices.to(torch.int32)
            w = torch.full((m, TOP_K), 0.5, device="cuda")
            out = torch.empty((m, FOUT), device="cuda")
            if grouped:
                ws = bestla.moe_grouped_workspace_alloc(gate, up, down, m, TOP_K)

                def fn():
                    bestla.moe_ffn_grouped(gate, up, down, x, ids, w, out=out, stream=s, workspace=ws)
            else:
                ws = bestla.moe_workspace_alloc(m, TOP_K, FMID, FOUT)

                def fn():
                    bestla.moe_ffn(gate, up, down, x, ids, w, out=out, stream=s, workspace=ws)
            for _ in range(WARM):
                fn()
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            t1 = time.perf_counter()
            s.synchronize()
            t2 = time.perf_counter()
            res[name] = {"us_per_call": round((t2 - t0) * 1e6 / CALLS, 3),
                         "us_enqueue": round((t1 - t0) * 1e6 / CALLS, 3), "sum": float(out.double().sum())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
