#!/usr/bin/env python3
"""Device code of two csrc trees, kernel by kernel, without a GPU.

    python tools/kernel_diff.py PARENT_CSRC NEW_CSRC [--flag FLAG]... [--work DIR] [--jobs N]

Every source of build.py's SOURCES in both directories is compiled to gfx950 assembly with build.py's FLAGS (without
-fPIC -shared, plus --offload-device-only -S).  Kernels are the entries of the code objects' metadata, matched by mangled
name.  Two kernels are identical when their instruction streams are, after comments are dropped and local labels are
renumbered in order of appearance, and their VGPR / AGPR / SGPR counts, static LDS, scratch and workgroup size agree.
The streams are compared as text: no instruction is looked for by name.  A kernel that differs is listed with the
opcodes whose counts differ.  Prints a markdown table (the figures are the second tree's); exit status 1 if any kernel
differs or exists in one tree only.  --work keeps the assembly there (default: a temporary directory).

--flag (repeatable) appends a compiler flag for both trees, so the search kernel's diagnostic builds can be compared as
well: --flag=-DCO_PROF, --flag=-DCO_COLD_NOINLINE, --flag=-DCO_SB=1 ...

The parent's tree: csrc/host.h includes ../../include/corintho_hip.h, so an export of the parent commit has to keep
include/ beside corintho_ai_amd/ --
    mkdir /tmp/parent && git archive HEAD~1 corintho_ai_amd include | tar -x -C /tmp/parent
    python tools/kernel_diff.py /tmp/parent/corintho_ai_amd/csrc corintho_ai_amd/csrc"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corintho_ai_amd import build as B  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "max_flat_workgroup_size")
LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def compile_tree(csrc, work, jobs, extra=()):
    """-> the assembly files of the tree's sources, compiled `jobs` at a time"""
    os.makedirs(work, exist_ok=True)
    flags = [f for f in B.FLAGS if f not in ("-fPIC", "-shared")] + ["--offload-device-only", "-S"] + list(extra)
    todo = [(os.path.join(csrc, s), os.path.join(work, s + ".s")) for s in B.SOURCES
            if os.path.exists(os.path.join(csrc, s))]  # (an earlier tree need not have every source of today's)
    running, done = [], []
    while todo or running:
        while todo and len(running) < jobs:
            src, out = todo.pop(0)
            running.append((subprocess.Popen([B.hipcc()] + flags + ["-o", out, src]), src, out))
        proc, src, out = running.pop(0)
        if proc.wait() != 0:
            raise RuntimeError("compiling %s failed" % src)
        done.append(out)
    return done


def parse(path, kernels):
    """adds {name: (instruction lines, metadata)} of one assembly file to `kernels`"""
    lines = open(path).read().split("\n")
    bodies, name = {}, None
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and not ln.startswith(".L"):
            name = m.group(1)
            bodies[name] = []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            name = None
            continue
        code = ln.split(";", 1)[0].strip()
        if code:
            bodies[name].append(code)
    meta, inside = [], False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and ln and not ln.startswith(" "):
            inside = False
        if not inside:
            continue
        m = re.match(r"^  (- |  )\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "- ":
            meta.append({})
        meta[-1][m.group(2)] = m.group(3).strip("'\"")
    for d in meta:
        n = d["name"]
        labels = {}
        body = [LOCAL.sub(lambda x: labels.setdefault(x.group(0), ".L%d" % len(labels)), c) for c in bodies[n]]
        kernels[n] = (body, tuple(int(d.get(k, 0)) for k in META))


def opcode_counts(body):
    return collections.Counter(c.split()[0] for c in body if not c.endswith(":") and not c.startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--flag", action="append", default=[], help="extra compiler flag for both trees (repeatable)")
    ap.add_argument("--work")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = a.work or tmp.name
    trees = []
    for label, csrc in (("parent", a.parent), ("new", a.new)):
        k = {}
        for s in compile_tree(csrc, os.path.join(work, label), a.jobs, a.flag):
            parse(s, k)
        trees.append(k)
    old, new = trees
    only = sorted(set(old) ^ set(new))
    print("%d kernels in the parent, %d in the new tree, %d only in one of them" % (len(old), len(new), len(only)))
    for n in only:
        print("only in %s: `%s`" % ("the parent" if n in old else "the new tree", n))
    print()
    print("| kernel | instructions | VGPR | AGPR | SGPR | LDS (B) | scratch | block | parent = new |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---|")
    differ = []
    for n in sorted(set(old) & set(new)):
        body, meta = new[n]
        same = old[n] == new[n]
        if not same:
            differ.append(n)
        ninstr = sum(opcode_counts(body).values())
        print("| `%s` | %d | %s | %s |" % (n, ninstr, " | ".join(str(v) for v in meta), "identical" if same else "**differs**"))
    for n in differ:
        co, cn = opcode_counts(old[n][0]), opcode_counts(new[n][0])
        print("\n`%s` differs.  %s parent %s, new %s.  Opcode counts (parent/new): %s" % (
            n, ", ".join(META), old[n][1], new[n][1],
            ", ".join("`%s` %d/%d" % (o, co[o], cn[o]) for o in sorted(set(co) | set(cn)) if co[o] != cn[o]) or "the same"))
    print("\n%d identical, %d differ" % (len(set(old) & set(new)) - len(differ), len(differ)))
    return 1 if differ or only else 0


if __name__ == "__main__":
    sys.exit(main())
