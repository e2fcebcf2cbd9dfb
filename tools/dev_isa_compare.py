"""Per-kernel ISA comparison of the working tree against a base commit (development tool, no GPU needed).

Compiles the device code of both trees with the product's flags (`hipcc <flags> --cuda-device-only -S`), the base from a temporary
`git worktree`, and compares every kernel of the base: its instructions (comments dropped and local label numbers normalised: both count
functions) and its kernel descriptor.  Kernels only the working tree has are listed with their VGPR count and scratch size.  Exit status 1 when a kernel of
the base differs or is missing.

    python tools/dev_isa_compare.py [--base main] [--keep DIR]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SOURCES = ["icp-variants_amd/csrc/icp_hip.hip", "icp-variants_amd/csrc/icp_batch.hip"]


def compile_tree(tree, out_dir, tag):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-Wall")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    outs = []
    for src in SOURCES:
        out = os.path.join(out_dir, "%s_%s.s" % (tag, os.path.basename(src)))
        subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-w", "-I", os.path.join(tree, "include"), "-S", os.path.join(tree, src), "-o", out])
        outs.append(out)
    return outs


def kernels(asm_files):
    """{symbol: (normalised body, descriptor, num_vgpr, private_seg_size)} of every __global__ in the assembly."""
    res = {}
    for path in asm_files:
        text = open(path).read()
        sets = {}
        for name, field, val in re.findall(r"\.set (\S+?)\.(num_vgpr|private_seg_size), (\d+)", text):
            sets.setdefault(name, {})[field] = int(val)
        descs = dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S))
        bodies, cur = {}, None
        for line in text.split("\n"):                      # a kernel's text: from its label to the next .Lfunc_end
            if cur is None:
                m = re.match(r"(\S+):\s*(?:;.*)?$", line)
                if m and m.group(1) in descs:
                    cur = m.group(1); bodies[cur] = []
            elif line.startswith(".Lfunc_end"):
                cur = None
            else:
                bodies[cur].append(line)
        for name, lines in bodies.items():
            body = "\n".join(l for l in (re.sub(r"\s*;.*$", "", l) for l in lines) if l.strip())     # comments carry function numbers
            body = re.sub(r"\.LBB\d+_", ".LBB_", body)
            body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
            body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
            f = sets.get(name, {})
            res[name] = (body, descs[name], f.get("num_vgpr"), f.get("private_seg_size"))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--base", default="main", help="commit to compare against (default: main)")
    ap.add_argument("--keep", default=None, help="directory to keep the assembly files in")
    ap.add_argument("--reuse", action="store_true", help="compare the assembly already in --keep instead of compiling")
    a = ap.parse_args()
    out_dir = a.keep or tempfile.mkdtemp(prefix="isa_cmp_")
    os.makedirs(out_dir, exist_ok=True)
    if a.reuse:
        base = kernels([os.path.join(out_dir, "base_%s.s" % os.path.basename(f)) for f in SOURCES])
        head = kernels([os.path.join(out_dir, "head_%s.s" % os.path.basename(f)) for f in SOURCES])
    else:
        wt = tempfile.mkdtemp(prefix="isa_base_")
        os.rmdir(wt)
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", wt, a.base], stdout=subprocess.DEVNULL)
        try:
            base = kernels(compile_tree(wt, out_dir, "base"))
        finally:
            subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", wt])
        head = kernels(compile_tree(ROOT, out_dir, "head"))
    bad = 0
    for name in sorted(base):
        if name not in head:
            print("MISSING    %s" % name); bad += 1
        elif head[name][:2] != base[name][:2]:
            print("DIFFERENT  %s" % name); bad += 1
    print("%d kernels of %s: %d identical, %d different or missing" % (len(base), a.base, len(base) - bad, bad))
    for name in sorted(set(head) - set(base)):
        print("NEW        %s  vgpr %s  scratch %s" % (name, head[name][2], head[name][3]))
    if not a.keep:
        shutil.rmtree(out_dir, ignore_errors=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
