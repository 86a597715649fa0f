#!/usr/bin/env python3
"""Path-size report of the M = 1 decode GEMV kernels, without a GPU.

A decode launch pays for the code it executes where no memory latency hides it (the instruction cache starts cold on
every dispatch): everything before the first weight-tile load, and everything after the barrier.  This tool
cross-compiles csrc/woq_gemv.h for gfx950 (device code only, just the named instantiations, no launchers), disassembles
the object and prints, per kernel:

  preload          dwords of leading kernel arguments the hardware delivers in SGPRs at dispatch (the kernel
                   descriptor's kernarg preload length).  Where it is not 0 the code begins with a 256-byte
                   compatibility block (scalar loads of those arguments, a wait, a branch) that hardware with preload
                   support skips: the walk below starts at the real entry behind it
  pro_ins / pro_B  instructions and code bytes from the entry to the first non-temporal tile load on the live path
                   (the shortest path through the control-flow graph to a `buffer_load_dwordx4 ... offen ... nt`
                   whose offset register does not hold the out-of-range constant of a two-armed stage load's dead arm)
  lgkm / vm        s_waitcnt on that path with an lgkmcnt / a vmcnt field
  tail_B           code bytes from the (first) s_barrier to the last s_endpgm
  barriers         number of s_barrier instructions
  total_B          code bytes of the kernel
  sgpr / vgpr / scratch   from the code-object metadata

  python tools/gemv_path_bytes.py                 # the default list of the current tree
  python tools/gemv_path_bytes.py --set headline  # the two headline instantiations only
  python tools/gemv_path_bytes.py --source OTHER/woq_gemv.hip --legacy   # a tree without the specialised kernel
  python tools/gemv_path_bytes.py --against OTHER/woq_gemv.hip           # both sources, row by row, and per kernel
                                                                         # whether their instruction streams are equal
"""
import argparse
import difflib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT = {"f32": 0, "f16": 1, "bf16": 2}


def generic(bits, gpt, at, asym, ksn, spw, batch, nst, st=-1):
    """woq_gemv_m1_kernel: the full-GemvArgs kernel with the runtime epilogue switch."""
    b = lambda v: "true" if v else "false"
    return "woq_gemv_m1_kernel<%d,%d,%d,%s,%d,%d,%s,%d,%d>" % (bits, gpt, ACT[at], b(asym), ksn, spw, b(batch), nst, st), \
        "GemvArgs"


def spec(bits, gpt, at, asym, ksn, spw, nst, st, nwt, nsc, ahead=False):
    """woq_gemv_m1s_kernel: preloaded leading arguments, weight count / slots per column / epilogue class at compile
    time; ahead: its load-ahead order."""
    b = lambda v: "true" if v else "false"
    return "woq_gemv_m1s_kernel<%d,%d,%d,%s,%d,%d,%d,%d,%d,%d%s>" % (bits, gpt, ACT[at], b(asym), ksn, spw, nst, st, nwt,
                                                                     nsc, ",true" if ahead else ""), \
        "const void*, const void*, const void*, const void*, const void*, int, uint32_t, uint32_t, int, GemvM1Rest<%d>" % nwt


# name -> (kernel template-id, argument type).  Llama-2-7B int4 g128 decode: QKV (3 weights), O (1), gate/up (pair) run
# 16 waves of one 2-tile slice each; down (K = 11008) runs 4-tile slices; lm_head two register stages.
def kernel_sets(legacy):
    if legacy:
        head = [("qkv/o/gate-up", generic(4, 1, "f32", False, 2, 1, False, 1)),
                ("down", generic(4, 1, "f32", False, 4, 2, False, 1))]
        rest = [("lm_head", generic(4, 1, "f32", False, 2, 1, False, 2))]
    else:
        head = [("o (1 weight)", spec(4, 1, "f32", False, 2, 1, 1, -1, 1, 16)),
                ("down", spec(4, 1, "f32", False, 4, 2, 1, -1, 1, 11))]
        rest = [("qkv (3 weights)", spec(4, 1, "f32", False, 2, 1, 1, -1, 3, 16)),
                ("gate/up (pair)", spec(4, 1, "f32", False, 2, 1, 1, -1, 2, 16)),
                ("lm_head", spec(4, 1, "f32", False, 2, 1, 2, -1, 1, 16)),
                ("asym (spec)", spec(4, 1, "f32", True, 2, 1, 1, -1, 1, 16)),
                ("generic qkv/o/gate-up", generic(4, 1, "f32", False, 2, 1, False, 1)),
                ("generic down", generic(4, 1, "f32", False, 4, 2, False, 1))]
    rest += [("asym/bf16-scale (generic)", generic(4, 1, "f32", True, 2, 1, False, 1)),
             ("batched", generic(4, 1, "f32", False, 2, 1, True, 3))]
    # the load-ahead forms (woq_gemv_s6.hip), each behind the present form of the same launch
    ahead = []
    if not legacy:
        for label, asym, ksn, spw, nwt, nsc in (("qkv (3 weights)", False, 2, 1, 3, 16), ("gate/up (pair)", False, 2, 1, 2, 16),
                                                ("one weight", False, 2, 1, 1, 16),
                                                ("asym qkv", True, 2, 1, 3, 16), ("asym gate/up", True, 2, 1, 2, 16),
                                                ("asym one weight", True, 2, 1, 1, 16)):
            ahead += [(label, spec(4, 1, "f32", asym, ksn, spw, 1, -1, nwt, nsc)),
                      (label + " ahead", spec(4, 1, "f32", asym, ksn, spw, 1, -1, nwt, nsc, True))]
    return {"headline": head, "all": head + rest, "ahead": ahead}


def find_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def hipcc_path():
    p = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    return p if os.path.exists(p) else shutil.which("hipcc")


def compile_kernels(source, kernels, workdir, arch="gfx950"):
    """Device-only object holding exactly `kernels` [(template-id, arg type)]; returns its path.  `source` may be a
    tree's woq_gemv.hip in either layout: where woq_gemv.h lies beside it, the kernels are there and the .hip holds
    launchers that would instantiate an object's worth of them."""
    header = os.path.splitext(source)[0] + ".h"
    if source.endswith(".hip") and os.path.exists(header):
        source = header
    wrap = os.path.join(workdir, "gemv_only.hip")
    with open(wrap, "w") as f:
        f.write('#include "%s"\nnamespace nad {\n' % os.path.abspath(source))
        for tid, arg in kernels:
            f.write("template __global__ void %s(%s);\n" % (tid, arg))
        f.write("}\n")
    obj = os.path.join(workdir, "gemv_only.o")
    # GEMV_PART=99: for an older tree's woq_gemv.hip, whose launcher section (it would instantiate every kernel of
    # the object) that value leaves out; csrc/woq_gemv.h holds no launchers and does not read it
    # the preload flag of the Makefile's GEMV_PRELOAD (kernels whose first parameter is a struct keep length 0)
    cmd = [hipcc_path(), "--offload-arch=" + arch, "--cuda-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17",
           "-mllvm", "-amdgpu-kernarg-preload-count=14", "-DGEMV_PART=99", "-I", os.path.dirname(os.path.abspath(source)), "-Wno-unused-function", "-c", wrap, "-o", obj]
    subprocess.run(cmd, check=True)
    return obj


INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):((?:\s+[0-9A-Fa-f]{8})+)\s*$")
LABEL = re.compile(r"^([0-9a-f]+) <(.+)>:$")


def disassemble(obj):
    """{symbol: [(addr, size, mnemonic, operands)]} of the kernels (their local labels folded in)."""
    out = subprocess.run([find_tool("llvm-objdump"), "-d", "--demangle", obj], check=True, capture_output=True,
                         text=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = LABEL.match(line)
        if m:
            if not m.group(2).startswith("L") and "BB" not in m.group(2).split("(")[0]:
                cur = funcs.setdefault(m.group(2), [])
            continue
        m = INS.match(line)
        if m and cur is not None:
            words = m.group(4).split()
            cur.append((int(m.group(3), 16), 4 * len(words), m.group(1), m.group(2)))
    return funcs


def metadata(obj):
    """{symbol-ish name: dict(sgpr, vgpr, scratch)} from the code-object notes."""
    out = subprocess.run([find_tool("llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    res, cur = [], {}
    for line in out.splitlines():
        line = line.strip().lstrip("- ")
        for key in (".name:", ".sgpr_count:", ".vgpr_count:", ".private_segment_fixed_size:", ".agpr_count:"):
            if line.startswith(key):
                if key == ".name:" and ("woq_gemv" not in line):
                    continue
                cur[key[1:-1]] = line[len(key):].strip()
        if line.startswith(".wavefront_size:") and cur:
            res.append(cur)
            cur = {}
    return res


def preload_lengths(obj):
    """{mangled kernel name: kernarg preload length in dwords} from the kernel descriptors (the <name>.kd objects: 64
    bytes, the preload field is the u16 at byte 58, length in its bits 0-6)."""
    with open(obj, "rb") as f:
        d = f.read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    res = {}
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for o in range(sec[4], sec[4] + sec[5], 24):
            name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, o)
            name = d[stroff + name_off:d.index(b"\0", stroff + name_off)].decode()
            if not name.endswith(".kd") or not 0 < shndx < shnum:
                continue
            at = secs[shndx][4] + value - secs[shndx][3]
            res[name[:-3]] = struct.unpack_from("<H", d, at + 58)[0] & 0x7F
    return res


def analyse(ins, preload=0):
    """Path figures of one kernel's instruction list; preload: its kernarg preload length."""
    by_addr = {a: i for i, (a, _, _, _) in enumerate(ins)}
    base = ins[0][0]
    # the real entry: behind the 256-byte block for hardware without kernarg preload
    entry = by_addr[base + 256] if preload else 0

    def target(i):
        a, sz, mn, ops = ins[i]
        m = re.match(r"\s*(-?\d+)", ops)  # s_branch simm16 (dwords relative to the next instruction)
        if m is None:
            return None
        return by_addr.get(a + sz + 4 * int(m.group(1)))

    def is_tile_load(i):
        _, _, mn, ops = ins[i]
        if not (mn == "buffer_load_dwordx4" and " nt" in (" " + ops) and "offen" in ops):
            return False
        # the out-of-range arm of a two-armed stage load: its offset register was last written (in program order) by a
        # move of the out-of-range constant
        voff = ops.split(",")[1].strip()
        for k in range(i - 1, -1, -1):
            dst = ins[k][3].split(",")[0].strip()
            if dst == voff and ins[k][2].startswith("v_"):
                return not (ins[k][2].startswith("v_mov_b32") and "0x7fff0000" in ins[k][3])
        return True

    # shortest path (in instructions) from the entry to a live tile load: Dijkstra over instruction indices
    import heapq
    dist, prev, heap, goal = {entry: 0}, {}, [(0, entry)], None
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist.get(i, 1 << 60):
            continue
        if is_tile_load(i):
            goal = i
            break
        mn = ins[i][2]
        nxt = []
        if mn == "s_endpgm":
            continue
        if mn == "s_branch":
            nxt = [target(i)]
        elif mn.startswith("s_cbranch"):
            nxt = [i + 1, target(i)]
        else:
            nxt = [i + 1]
        for j in nxt:
            if j is None or j >= len(ins):
                continue
            if d + 1 < dist.get(j, 1 << 60):
                dist[j] = d + 1
                prev[j] = i
                heapq.heappush(heap, (d + 1, j))
    r = {"preload": preload, "pro_ins": -1, "pro_B": -1, "lgkm": -1, "vm": -1}
    if goal is not None:
        path, i = [], goal
        while i != entry:
            i = prev[i]
            path.append(i)
        path.reverse()
        r["pro_ins"] = len(path)
        r["pro_B"] = sum(ins[i][1] for i in path)
        waits = [ins[i][3] for i in path if ins[i][2] == "s_waitcnt"]
        r["lgkm"] = sum("lgkmcnt" in w for w in waits)
        r["vm"] = sum("vmcnt" in w for w in waits)
    bars = [i for i, x in enumerate(ins) if x[2] == "s_barrier"]
    ends = [i for i, x in enumerate(ins) if x[2] == "s_endpgm"]
    r["barriers"] = len(bars)
    r["tail_B"] = (ins[ends[-1]][0] + ins[ends[-1]][1] - ins[bars[0]][0]) if bars and ends else -1
    r["total_B"] = ins[-1][0] + ins[-1][1] - base
    r["total_ins"] = len(ins)
    return r


def squash(s):
    return re.sub(r"\s+", "", s).replace("(nad::ActType)", "").replace("nad::", "")


def report(source, kernels, arch="gfx950", keep=None, with_code=False):
    """[(label, template-id, figures dict)] for `kernels` [(label, (template-id, arg type))]; with_code appends each
    kernel's instruction stream [(mnemonic, operands)] (no addresses, no encodings) to its row."""
    work = keep or tempfile.mkdtemp(prefix="gemv_path_")
    try:
        obj = compile_kernels(source, [k for _, k in kernels], work, arch)
        funcs = disassemble(obj)
        meta = metadata(obj)
        pre = preload_lengths(obj)
        rows = []
        for label, (tid, _) in kernels:
            key = squash(tid)
            # demangled symbols spell bools / enums differently between versions: match on the template arguments
            args = re.findall(r"-?\d+|true|false", key.split("<", 1)[1])
            name = key.split("<")[0]

            def same(sym):
                s = squash(sym)
                if not s.startswith("void" + name + "<") and not s.startswith(name + "<"):
                    return False
                got = re.findall(r"-?\d+|true|false", s.split("<", 1)[1].split(">(")[0])
                return got == args or got == args + ["false"]  # a trailing template parameter left at its default

            sym = [s for s in funcs if same(s)]
            if len(sym) != 1:
                raise RuntimeError("kernel %s: %d symbols match" % (tid, len(sym)))
            rows.append([label, tid, None, sym[0]])
        # metadata entries come in the order of the kernels' definition = the order of explicit instantiation
        if len(meta) == len(rows):
            order = sorted(range(len(rows)), key=lambda i: funcs[rows[i][3]][0][0])
            for mi, ri in enumerate(order):
                rows[ri][2] = analyse(funcs[rows[ri][3]], pre[meta[mi]["name"]])
                rows[ri][2].update(sgpr=int(meta[mi]["sgpr_count"]), vgpr=int(meta[mi]["vgpr_count"]),
                                   scratch=int(meta[mi]["private_segment_fixed_size"]))
        else:
            raise RuntimeError("metadata entries (%d) do not match the kernels (%d)" % (len(meta), len(rows)))
        if with_code:
            return [(l, t, f, [(mn, re.sub(r"\s+", " ", ops)) for _, _, mn, ops in funcs[sym]]) for l, t, f, sym in rows]
        return [(l, t, f) for l, t, f, _ in rows]
    finally:
        if keep is None:
            shutil.rmtree(work, ignore_errors=True)


COLS = ["preload", "pro_ins", "pro_B", "lgkm", "vm", "tail_B", "barriers", "total_ins", "total_B", "sgpr", "vgpr", "scratch"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(ROOT, "neural_amd", "csrc", "woq_gemv.h"))
    ap.add_argument("--set", default="all", choices=["all", "headline", "ahead"])
    ap.add_argument("--legacy", action="store_true", help="the source has no woq_gemv_m1s_kernel: list the generic ones")
    ap.add_argument("--keep", default=None, help="directory to keep the wrapper source and the object in")
    ap.add_argument("--against", default=None, metavar="OTHER/woq_gemv.hip",
                    help="compile the same instantiations from this source too: both rows per kernel, and whether the "
                         "two instruction streams (mnemonics and operands) are identical")
    args = ap.parse_args()
    if hipcc_path() is None:
        sys.exit("hipcc not found")
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
    kernels = kernel_sets(args.legacy)[args.set]
    head = "%-28s " % "kernel" + " ".join("%9s" % c for c in COLS)
    if args.against is None:
        rows = report(args.source, kernels, keep=args.keep)
        print("# %s" % os.path.relpath(args.source, ROOT))
        print(head + "  instantiation")
        for label, tid, f in rows:
            print("%-28s " % label + " ".join("%9d" % f[c] for c in COLS) + "  " + tid)
        return
    mine = report(args.source, kernels, keep=args.keep, with_code=True)
    other = report(args.against, kernels, with_code=True)
    print("# a: %s\n# b: %s" % (os.path.relpath(args.source, ROOT), os.path.relpath(args.against, ROOT)))
    print(head + "  code")
    for (label, tid, fa, ca), (_, _, fb, cb) in zip(mine, other):
        print("%-28s " % label + "  " + tid)
        if ca == cb:
            verdict = "identical"
        else:  # how far apart: instructions of the longer stream outside the longest common subsequence blocks
            same = sum(b.size for b in difflib.SequenceMatcher(None, ca, cb, autojunk=False).get_matching_blocks())
            verdict = "DIFFERS (%d of %d instructions)" % (max(len(ca), len(cb)) - same, max(len(ca), len(cb)))
        print("%-28s " % "  a" + " ".join("%9d" % fa[c] for c in COLS) + "  " + verdict)
        print("%-28s " % "  b" + " ".join("%9d" % fb[c] for c in COLS))


if __name__ == "__main__":
    main()
