#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees of this project, kernel by kernel.

    python3 tools/compare_device_code.py OLD_TREE NEW_TREE [--dev] [--jobs N] [--objects a,b,c] [--out report.md]

For each tree the compile commands of the library's objects are taken from `make -n -B all` (with --dev: DEV=1), every
object is compiled again with `--offload-device-only -S`, and the assembly is split per kernel symbol into: instruction
text, the .amdhsa_kernel descriptor block and the kernel's metadata record (.vgpr_count, .sgpr_count, LDS, scratch, ...).
The only thing normalised is the per-compilation `__hip_cuid_<hash>` symbol.  Objects are matched by name, so a kernel that
moves to another object shows up as missing in one and new in the other.  --objects restricts both trees to the named
objects (for example born,rdm,pauli,gates,wgate,measure).
Exit status 0 when every object emits the same kernel symbols in both trees and every kernel is identical (--dev: equal
names and register counts).
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile


def compile_commands(tree, dev):
    out = subprocess.run(["make", "-n", "-B", "all"] + (["DEV=1"] if dev else []), cwd=tree, check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        w = shlex.split(line)
        if "-c" in w and "-o" in w:
            cmds[os.path.basename(w[w.index("-o") + 1])[:-2]] = w
    return cmds


def emit_asm(tree, unit, words, tmp):
    dst = os.path.join(tmp, unit + ".s")
    w = list(words)
    w[w.index("-o") + 1] = dst
    w[w.index("-c")] = "-S"
    subprocess.run(w + ["--offload-device-only"], cwd=tree, check=True, capture_output=True)
    with open(dst) as f:
        return unit, re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read())


def split_kernels(asm):
    """{symbol: (text, descriptor, metadata)}"""
    lines = asm.split("\n")
    desc, text, meta = {}, {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = "\n".join(lines[i:j + 1])
            i = j
        i += 1
    for sym in desc:
        a = next(n for n, l in enumerate(lines) if l.startswith(sym + ":"))
        b = a
        while not re.match(r"\.Lfunc_end\d+:", lines[b]):
            b += 1
        text[sym] = "\n".join(lines[a:b])
    if "amdhsa.kernels:" in lines:
        i = lines.index("amdhsa.kernels:") + 1
        rec = []
        while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
            if lines[i].startswith("  - ") and rec:
                meta[re.search(r"\.name:\s+(\S+)", "\n".join(rec)).group(1)] = "\n".join(rec)
                rec = []
            rec.append(lines[i])
            i += 1
        if rec:
            meta[re.search(r"\.name:\s+(\S+)", "\n".join(rec)).group(1)] = "\n".join(rec)
    return {s: (text[s], desc[s], meta.get(s, "")) for s in desc}


def tree_kernels(tree, dev, jobs, objects):
    """{(object, symbol): parts}: template instantiations that several objects emit (weak symbols) count once per object"""
    cmds = compile_commands(tree, dev)
    if objects:
        missing = sorted(set(objects) - set(cmds))
        if missing:
            sys.exit("%s builds no object named %s" % (tree, ", ".join(missing)))
        cmds = {u: cmds[u] for u in objects}
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for unit, asm in ex.map(lambda kv: emit_asm(tree, kv[0], kv[1], tmp), sorted(cmds.items())):
            for sym, parts in split_kernels(asm).items():
                kernels[(unit, sym)] = parts
    return kernels, sorted(cmds)


def regs(meta):
    return tuple(int(re.search(r"\.%s:\s+(\d+)" % k, meta).group(1)) for k in ("vgpr_count", "sgpr_count", "agpr_count"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--dev", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--objects", type=lambda v: [u for u in v.split(",") if u], help="compare only these objects, e.g. born,rdm")
    ap.add_argument("--out")
    a = ap.parse_args()
    ko, uo = tree_kernels(a.old, a.dev, a.jobs, a.objects)
    kn, un = tree_kernels(a.new, a.dev, a.jobs, a.objects)
    rep = ["## %s build" % ("Development (`make dev`)" if a.dev else "Product (`make`)"), ""]
    rep.append("| object | kernels, old tree | kernels, new tree |")
    rep.append("|---|---|---|")
    for u in sorted(set(uo) | set(un)):
        rep.append("| %s | %s | %s |" % (u, sum(1 for k in ko if k[0] == u) if u in uo else "-", sum(1 for k in kn if k[0] == u) if u in un else "-"))
    rep.append("| **all** | %d | %d |" % (len(ko), len(kn)))
    rep.append("")
    only_old, only_new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    rep.append("(object, kernel symbol) pairs only in the old tree: %s.  Only in the new tree: %s." %
               (", ".join("%s: `%s`" % k for k in only_old) or "none", ", ".join("%s: `%s`" % k for k in only_new) or "none"))
    bad = []
    for s in sorted(set(ko) & set(kn)):
        parts = [n for n, x, y in zip(("instruction text", "descriptor", "metadata"), ko[s], kn[s]) if x != y]
        if regs(ko[s][2]) != regs(kn[s][2]):
            bad.append("%s: `%s`: registers (vgpr, sgpr, agpr) %s -> %s" % (s + (regs(ko[s][2]), regs(kn[s][2]))))
        elif parts and not a.dev:
            bad.append("%s: `%s`: %s differ" % (s + (", ".join(parts),)))
    same = len(set(ko) & set(kn)) - len(bad)
    rep.append("")
    rep.append("%d of %d common kernels %s." % (same, len(set(ko) & set(kn)),
                                            "have equal register counts" if a.dev else "are identical in instruction text, .amdhsa_kernel descriptor and metadata record"))
    rep += ["", "Kernels that differ:", ""] + ["- " + b for b in bad] if bad else ["No kernel differs."]
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 1 if (bad or only_old or only_new) else 0


if __name__ == "__main__":
    sys.exit(main())
