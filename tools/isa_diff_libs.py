#!/usr/bin/env python3
"""Two builds of the library, kernel by kernel: is the instruction stream the same?

The gfx950 code object of each library (tools/occupancy.py takes it out of the .so) is disassembled with llvm-objdump; every kernel's
instructions are compared after the addresses are stripped (the leading address and encoding of a line, the pc-relative literals
behind s_getpc_b64, branch targets printed as addresses).  Kernels are matched by the sheet's names (occupancy.short), so a STag
kernel's frame-at-a-time form keeps its name whether it is a named kernel or k_stag_frame<k_stag_X_fn, ...>.  Per kernel:
    same         the same instructions in the same order
    reordered    the same multiset of instructions once register NUMBERS are blanked (v12 -> v#): scheduling or register choice
    differs      anything else -- with both instruction counts
Runs anywhere (no GPU).  Usage: isa_diff_libs.py <parent.so> <new.so> > profiles/<name>_isa.txt"""
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _occ():
    spec = importlib.util.spec_from_file_location("occupancy", os.path.join(ROOT, "tools", "occupancy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(lib):
    """sheet name -> list of instruction texts, for every kernel (symbol with a .kd descriptor) of the library"""
    occ = _occ()
    with tempfile.TemporaryDirectory() as td:
        co = occ.code_object(lib, td)
        names = set(occ.read_notes(co))
        txt = subprocess.check_output([f"{occ.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    dm = occ.demangle(sorted(names))
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(occ.short(dm[m.group(1)]), []) if m.group(1) in names else None
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", line.strip())
        ins = re.sub(r"\s+", " ", ins)
        if not ins or ins == "...":  # (zero padding between functions)
            continue
        cur.append(ins)
    for body in out.values():
        # the two literals that follow s_getpc_b64 are distances to a symbol: they move with the layout of the object
        for i, ins in enumerate(body):
            if ins.startswith("s_getpc_b64"):
                for j in (i + 1, i + 2):
                    if j < len(body) and re.match(r"s_add(c)?_u32 ", body[j]):
                        body[j] = re.sub(r", (0x[0-9a-f]+|\d+)$", ", <pcrel>", body[j])
        while body and body[-1].startswith(("s_code_end", "s_nop")):  # (padding behind s_endpgm)
            body.pop()
    return out


def blank(ins):
    if re.match(r"s_c?branch", ins):  # (a relative target moves with every instruction added or dropped between it and the branch)
        return ins.split(" ")[0] + " <target>"
    return re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", ins)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"# parent: {len(a)} kernels, new: {len(b)} kernels")
    for n in sorted(set(a) - set(b)):
        print(f"only in parent  {n}  ({len(a[n])} instructions)")
    for n in sorted(set(b) - set(a)):
        print(f"only in new     {n}  ({len(b[n])} instructions)")
    tally = collections.Counter()
    for n in sorted(set(a) & set(b)):
        stag = n.startswith("k_stag_")
        if a[n] == b[n]:
            kind = "same"
        elif collections.Counter(map(blank, a[n])) == collections.Counter(map(blank, b[n])):
            kind = "reordered"
        else:
            kind = "differs"
        tally[("stag " if stag else "other ") + kind] += 1
        if kind != "same" or stag:
            extra = ""
            if kind == "differs":
                d = collections.Counter(map(blank, b[n]))
                d.subtract(collections.Counter(map(blank, a[n])))
                ch = sorted((k, v) for k, v in d.items() if v)
                extra = "  | " + "; ".join(f"{'+' if v > 0 else ''}{v} {k}" for k, v in ch[:12]) + (" ..." if len(ch) > 12 else "")
            print(f"{kind:10s} {n}  {len(a[n])} -> {len(b[n])} instructions{extra}")
    print("# " + ", ".join(f"{k}: {v}" for k, v in sorted(tally.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
