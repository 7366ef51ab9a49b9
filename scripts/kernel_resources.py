#!/usr/bin/env python3
"""Registers, spills, scratch, LDS and occupancy of every kernel of libqgd_amd.so, one line per kernel, as the compiler reports them.

    python scripts/kernel_resources.py > profiles/kernel_resources.txt
        compiles qgdsolver_amd/csrc into a temporary directory with -Rpass-analysis=kernel-resource-usage and prints the table.
    python scripts/kernel_resources.py --compare OLD.so NEW.so [--mnemonics] [--gained-parameter] [--multiset]
        disassembles the gfx950 code objects of two builds of the library kernel by kernel: lists the kernels only one of them has and
        those whose instructions differ (encodings and operands; with --mnemonics the sequence of mnemonics only, for a change that
        moves kernel-argument offsets).  Exit status 1 when a common kernel differs.  How a refactor shows that it left the device
        code alone.  --gained-parameter: a kernel of OLD that NEW only has with one more, trailing template argument is compared with
        the instantiation whose new argument is 0 (`k<3>` with `k<3, 0>`, `k` with `k<0>`): a compile-time flag was added and 0 is the
        code as it was.  --multiset: also compares, for every common kernel, HOW MANY of each mnemonic it has (s_waitcnt and s_nop
        left out) and lists the kernels where the counts differ: a change that shares or moves code without touching the arithmetic keeps
        every count (the same FMA / mul / add instructions: the same contraction, the same bits).

No GPU needed.  ROCM_PATH (default /opt/rocm) locates hipcc and the LLVM tools."""
import collections
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
          ("ScratchSize [bytes/lane]", "scratch_B"), ("LDS Size [bytes/block]", "lds_B"), ("Occupancy [waves/SIMD]", "occupancy")]


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def resource_table():
    with tempfile.TemporaryDirectory() as tmp:
        log = subprocess.run(["make", "-C", os.path.join(ROOT, "qgdsolver_amd", "csrc"), "ARCH=gfx950", "BUILD=" + os.path.join(tmp, "b"),
                              "OUT=" + os.path.join(tmp, "lib.so"), "EXTRA=-Rpass-analysis=kernel-resource-usage"],
                             capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in log.split("\n"):
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z][^:]*): (\d+)) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1):
            cur = kernels.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2)] = int(m.group(3))
    names = demangle(sorted(kernels))
    rows = sorted((names[k], v) for k, v in kernels.items() if "Occupancy [waves/SIMD]" in v)
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "qgdsolver_amd/csrc"], capture_output=True, text=True).stdout.strip()
    print(f"# kernels of libqgd_amd.so for gfx950: {len(rows)}; source: {'working tree on top of ' if dirty else ''}commit {head}")
    print("# command: python scripts/kernel_resources.py   (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")
    print("# " + " ".join(short for _, short in FIELDS) + " kernel")
    for name, v in rows:
        print(" ".join(f"{v[key]:>{len(short)}}" for key, short in FIELDS) + "   " + name)
    for title, pick in (("VGPRs spilled to scratch", lambda v: v["VGPRs Spill"]),
                        ("SGPRs spilled to VGPR lanes, no VGPR spill", lambda v: v["SGPRs Spill"] and not v["VGPRs Spill"]),
                        ("scratch without a spill (private arrays indexed at run time)", lambda v: v["ScratchSize [bytes/lane]"] and not v["VGPRs Spill"])):
        hit = [n for n, v in rows if pick(v)]
        print(f"# {title}: {len(hit)}" + "".join("\n#   " + n for n in hit))


def code_objects(lib):
    """the gfx950 members of every offload bundle in the library (one per translation unit)"""
    data, magic, out = open(lib, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", []
    at = data.find(magic)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + 24)
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple:
                out.append(data[at + off:at + off + size])
        at = data.find(magic, at + 1)
    return out


def kernel_disassembly(lib, mnemonics):
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"{i}.co")
            open(path, "wb").write(co)
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", path], capture_output=True, text=True, check=True).stdout
            funcs = {l.split()[-1] for l in syms.split("\n") if " FUNC " in l and " GLOBAL " in l or " FUNC " in l and " WEAK " in l}
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.split("\n"):
                m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    cur = kernels.setdefault(m.group(1), []) if m.group(1) in funcs else None
                elif cur is not None and line.startswith("\t"):
                    ins, _, enc = line.strip().partition("//")
                    if ins.strip() == "...":   # objdump's mark for zero bytes behind the last instruction (alignment of the next symbol)
                        continue
                    # (the address in front of the encoding goes: a kernel may move inside its code object; so does the kernel's own name in
                    # the note behind a branch, `<name+0x78>` -> `<+0x78>`: with --gained-parameter the name differs, the target does not)
                    cur.append(ins.split()[0] if mnemonics else ins.strip() + " |" + re.sub(r"<[^<>+\s]+(\+0x[0-9a-f]+)?>\s*$", r"<\1>", enc.partition(":")[2]))
    return kernels


def as_before_the_flag(name):
    """demangled `k<3, 0>(...)` -> `k<3>(...)`, `k<0>(...)` -> `k(...)` (an instantiated kernel template prints its return type)"""
    m = re.search(r"<([^<>]*)>\(", name)   # the first `<...>(`: the kernel's own arguments, in front of its parameter list
    if not m:
        return None
    args = m.group(1).split(", ")
    if args[-1] != "0":
        return None
    head = re.sub(r"^void ", "", name[:m.start()]) + (f"<{', '.join(args[:-1])}>" if len(args) > 1 else "")
    return head + name[m.end() - 1:]


def compare(old, new, mnemonics, gained=False, multiset=False):
    a, b = kernel_disassembly(old, mnemonics), kernel_disassembly(new, mnemonics)
    names = demangle(sorted(set(a) | set(b)))
    if gained:
        plain = {re.sub(r"^void ", "", names[k]): k for k in set(a) - set(b)}
        moved = {}
        for k in set(b) - set(a):
            was = as_before_the_flag(names[k])
            if was in plain:
                moved[k] = plain[was]
        print(f"kernels of {old} found in {new} with a trailing template argument 0: {len(moved)}")
        for k, ko in sorted(moved.items(), key=lambda kv: names[kv[0]]):
            print("   ", names[ko], "->", names[k])
            b[ko] = b.pop(k)
    for title, only in (("only in " + old, set(a) - set(b)), ("only in " + new, set(b) - set(a))):
        print(f"{title}: {len(only)}")
        for k in sorted(only, key=names.get):
            print("   ", names[k])
    differ = sorted((k for k in set(a) & set(b) if a[k] != b[k]), key=names.get)
    what = "sequence of mnemonics" if mnemonics else "instructions (operands and encodings)"
    print(f"in both: {len(set(a) & set(b))}; same {what}: {len(set(a) & set(b)) - len(differ)}; different: {len(differ)}")
    for k in differ:
        print("   ", names[k], f"({len(a[k])} -> {len(b[k])} instructions)")
    if multiset:
        count = lambda ins: collections.Counter(i.split()[0] for i in ins if i.split()[0] not in ("s_waitcnt", "s_nop"))
        odd = [(k, count(a[k]), count(b[k])) for k in differ if count(a[k]) != count(b[k])]
        print(f"different multiset of mnemonics (s_waitcnt, s_nop left out): {len(odd)}")
        for k, ca, cb in odd:
            print("   ", names[k], " ".join(f"{m} {ca[m]}->{cb[m]}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], "--mnemonics" in sys.argv[4:], "--gained-parameter" in sys.argv[4:], "--multiset" in sys.argv[4:]))
    resource_table()
