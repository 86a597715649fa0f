#!/usr/bin/env python3
"""Kernel by kernel, is the gfx950 machine code of two builds the same?  No GPU needed.

  python tools/kernel_code_diff.py OLD/build NEW/build [object stems ...]

Both arguments are object directories of neural_amd/Makefile (or single .o files).  For every object present in both
(or the named stems, e.g. woq_gemm7 woq_gemm_mid) the gfx950 code object is extracted and every kernel -- a function
symbol with a kernel descriptor `<symbol>.kd` -- is compared by

  * the bytes of its code, and
  * its descriptor: the 64 descriptor bytes less the entry offset, and the metadata's VGPR / AGPR / SGPR counts,
    scratch (private segment), static LDS (group segment) and kernarg size.

A kernel of b whose own template-id is one of a's plus a trailing `false` (a template parameter added at its default)
is compared with that kernel of a.  Nothing here looks for particular instructions.  Output: one line per object (kernels in a / in b / identical), then
every kernel that differs or exists on one side only, with its instruction and byte counts and registers on both
sides.  Exit status 1 if any kernel present on both sides differs.
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size")


def tool(name):
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (root + "/llvm/bin", root + "/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def unbundle(obj, work):
    """-> the gfx950 code object embedded in a host object (its .hip_fatbin bundle), or None for a host-only one"""
    link = os.path.join(work, "%d_%s" % (len(os.listdir(work)), os.path.basename(obj)))
    os.symlink(os.path.abspath(obj), link)  # llvm-objdump writes the bundle's entries next to its input
    subprocess.run([tool("llvm-objdump"), "--offloading", link], check=True, capture_output=True)
    out = link + ".0." + TARGET
    return out if os.path.exists(out) else None


def kernels(co):
    """{mangled name: dict(code=bytes, kd=bytes, + META)} of a code object"""
    with open(co, "rb") as f:
        d = f.read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    syms = {}
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for o in range(sec[4], sec[4] + sec[5], 24):
            name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, o)
            if not 0 < shndx < shnum:
                continue
            name = d[stroff + name_off:d.index(b"\0", stroff + name_off)].decode()
            at = secs[shndx][4] + value - secs[shndx][3]
            syms[name] = d[at:at + size]
    res = {n[:-3]: {"code": syms[n[:-3]], "kd": kd[:16] + kd[24:]} for n, kd in syms.items()
           if n.endswith(".kd") and n[:-3] in syms}
    notes = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    cur = {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) in META:
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == "symbol":
            cur["symbol"] = m.group(2).strip().strip("'\"")
        elif m.group(1) == "wavefront_size":  # the last key of a kernel's entry
            k = cur.get("symbol", "")[:-3]
            if k in res:
                res[k].update({key: cur.get(key, 0) for key in META})
            cur = {}
    return res


def instructions(co, sym):
    out = subprocess.run([tool("llvm-objdump"), "-d", "--disassemble-symbols=" + sym, co], check=True,
                         capture_output=True, text=True).stdout
    return sum(1 for line in out.splitlines() if re.search(r"//\s*[0-9A-Fa-f]+:(\s+[0-9A-Fa-f]{8})+\s*$", line))


def demangle(names):
    f = shutil.which("c++filt") or tool("llvm-cxxfilt")
    if not f or not names:
        return {n: n for n in names}
    out = subprocess.run([f], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def drop_trailing_false(name):
    """`ret kernel<..., false>(params)` -> `ret kernel<...>(params)`: only the last argument of the kernel's own
    template-id, found by matching brackets from the start of the name (nested template arguments and the parameter
    list are left alone); anything else is returned unchanged"""
    lt = name.find("<")
    depth = 0
    for i in range(lt, len(name)) if lt >= 0 else ():
        depth += name[i] == "<"
        depth -= name[i] == ">"
        if depth == 0:
            if name[i + 1:i + 2] == "(" and name[:i].endswith(", false"):
                return name[:i - len(", false")] + name[i:]
            break
    return name


def figures(co, sym, k):
    return "%6d ins %7d B  vgpr %3d agpr %3d sgpr %3d scratch %d lds %d kernarg %d" % (
        instructions(co, sym), len(k["code"]), k["vgpr_count"], k["agpr_count"], k["sgpr_count"],
        k["private_segment_fixed_size"], k["group_segment_fixed_size"], k["kernarg_segment_size"])


def objects(path):
    if os.path.isfile(path):
        return {os.path.basename(path)[:-2]: path}
    return {f[:-2]: os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".o")}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = objects(sys.argv[1]), objects(sys.argv[2])
    stems = sys.argv[3:] or [s for s in a if s in b]
    work = tempfile.mkdtemp(prefix="kdiff_")
    differs = 0
    try:
        for stem in stems:
            ca, cb = unbundle(a[stem], work), unbundle(b[stem], work)
            if ca is None or cb is None:
                continue  # a host-only object
            ka, kb = kernels(ca), kernels(cb)
            # a kernel template that gained a trailing parameter in b, left at `false`, is compared under its name in a
            dem = demangle([n for n in ka if n not in kb] + [n for n in kb if n not in ka])
            earlier = {dem[n]: n for n in ka if n not in kb}
            for n in [n for n in kb if n not in ka]:
                old = earlier.get(drop_trailing_false(dem[n]))
                if old is not None:
                    kb[old] = kb.pop(n)
            both = [n for n in ka if n in kb]
            diff = [n for n in both if ka[n] != kb[n]]
            only_a, only_b = [n for n in ka if n not in kb], [n for n in kb if n not in ka]
            print("%-16s a %4d  b %4d  identical %4d  differ %d  only a %d  only b %d" % (
                stem, len(ka), len(kb), len(both) - len(diff), len(diff), len(only_a), len(only_b)))
            names = demangle(diff + only_a + only_b)
            for n in diff:
                differs += 1
                print("  DIFFERS %s\n    a %s\n    b %s" % (names[n], figures(ca, n, ka[n]), figures(cb, n, kb[n])))
            for n in only_a:
                print("  only a  %s" % names[n])
            for n in only_b:
                print("  only b  %s" % names[n])
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("%d kernels differ" % differs)
    sys.exit(1 if differs else 0)


if __name__ == "__main__":
    main()
