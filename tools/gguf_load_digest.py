"""What the GGUF load entries put on the device, as digests: the fixture of tests/test_gguf_load_gpu.py.

For each of Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 (n = 17, k = 160: a second stripe of one real column, an int4 K tile and a
quarter / two int8 K tiles and a half) and Q6_K (n = 17, k = 512) the type's own C entry loads seeded blocks into a
device buffer of need + 256 bytes pre-filled with 0xA5, and record() returns the layout bytes, the guard bytes, the 14
values of nad_weight_info2, nad_device_get_compute and the M = 1 plan with the weight set to int8 mode, and the fp32
unpack.

  python tools/gguf_load_digest.py --write     (once, on a GPU, with the library of the commit the layouts are pinned to)

writes the blocks (tests/golden/gguf_load/<type>.blocks.bin) and manifest.txt: one line per type with the SHA-256 of
the layout bytes and of the unpack and the integers above.  Without --write it prints the same lines for the library
it runs on, so two builds can be compared by eye or by diff.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden", "gguf_load")
GUARD, FILL = 256, 0xA5

# name: GGUF type id, elements / bytes per block, byte offset of the fp16 d, of the fp16 m (None: no min), n, k
TYPES = {
    "q4_0": (2, 32, 18, 0, None, 17, 160),
    "q4_1": (3, 32, 20, 0, 2, 17, 160),
    "q5_0": (6, 32, 22, 0, None, 17, 160),
    "q5_1": (7, 32, 24, 0, 2, 17, 160),
    "q8_0": (8, 32, 34, 0, None, 17, 160),
    "q6_k": (14, 256, 210, 208, None, 17, 512),
}


def make_blocks(name):
    """seeded blocks: every code byte random, d in [1e-3, 1e-2] and m in [-0.5, 0.5] as fp16"""
    tid, be, bb, d_off, m_off, n, k = TYPES[name]
    rng = np.random.default_rng(1000 + tid)
    count = n * (k // be)
    b = rng.integers(0, 256, size=(count, bb), dtype=np.uint8)
    b[:, d_off:d_off + 2] = rng.uniform(1e-3, 1e-2, count).astype(np.float16).view(np.uint8).reshape(count, 2)
    if m_off is not None:
        b[:, m_off:m_off + 2] = rng.uniform(-0.5, 0.5, count).astype(np.float16).view(np.uint8).reshape(count, 2)
    return b.ravel()


def blocks_path(name):
    return os.path.join(GOLDEN, name + ".blocks.bin")


def entries(L, name):
    """the (size, load) closures of the type's own C entries: size(n, k), load(blocks, n, k, desc, mem, capacity, queue)"""
    tid = TYPES[name][0]
    if name == "q4_0":
        return L.nad_q4_0_device_size, L.nad_q4_0_device_load
    if name == "q6_k":
        return L.nad_q6_k_device_size, L.nad_q6_k_device_load
    return (lambda n, k: L.nad_gguf_device_size(tid, n, k)), (lambda *a: L.nad_gguf_device_load(tid, *a))


def record(name, blocks, entry=None):
    """load `blocks` through entry = (size, load) (default: the type's own entries) -> dict of what landed"""
    import torch
    from neural_amd import _lib, bestla
    L = _lib.lib()
    n, k = TYPES[name][5:7]
    size, load = entry or entries(L, name)
    need = size(n, k)
    assert need, _lib.last_error()
    mem = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    desc = (C.c_uint8 * L.bestla_device_storage_size())()
    queue = bestla._stream()
    rc = load(bestla._ptr(blocks), n, k, desc, bestla._ptr(mem), need, queue)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = mem.cpu().numpy()
    info = np.zeros(14, np.int64)
    assert L.nad_weight_info2(desc, bestla._ptr(info), 14) == 14, _lib.last_error()
    unpack = np.zeros((k, n), np.float32)
    assert L.nad_device_unpack_fp32(desc, bestla._ptr(unpack), queue) == 0, _lib.last_error()
    assert L.nad_device_set_compute(desc, 1) == 0, _lib.last_error()
    plan = np.zeros(6, np.int64)
    assert L.nad_plan_weight(desc, 1, 0, bestla._ptr(plan), 6) == 6, _lib.last_error()
    return dict(need=int(need), layout=host[:need], guard=host[need:], info=[int(v) for v in info],
                compute=int(L.nad_device_get_compute(desc)), plan=[int(v) for v in plan], unpack=unpack, mem=mem)


def manifest_line(name, r):
    return "%s need=%d layout=%s unpack=%s info=%s compute=%d plan=%s" % (
        name, r["need"], hashlib.sha256(r["layout"].tobytes()).hexdigest(),
        hashlib.sha256(r["unpack"].tobytes()).hexdigest(), ",".join(map(str, r["info"])), r["compute"],
        ",".join(map(str, r["plan"])))


def read_manifest():
    out = {}
    with open(os.path.join(GOLDEN, "manifest.txt")) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                out[line.split()[0]] = line.strip()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write the blocks and manifest.txt under tests/golden/gguf_load")
    ap.add_argument("--commit", default="", help="with --write: the commit the library was built from (a comment line)")
    args = ap.parse_args()
    lines = []
    for name in TYPES:
        if args.write:
            os.makedirs(GOLDEN, exist_ok=True)
            make_blocks(name).tofile(blocks_path(name))
        blocks = np.fromfile(blocks_path(name), np.uint8)
        r = record(name, blocks)
        assert (r["guard"] == FILL).all(), name
        lines.append(manifest_line(name, r))
    text = "\n".join(lines) + "\n"
    if args.write:
        with open(os.path.join(GOLDEN, "manifest.txt"), "w") as f:
            f.write("# tools/gguf_load_digest.py --write, library built from commit %s\n" % (args.commit or "?"))
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
