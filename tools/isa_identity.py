#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same, kernel by kernel?  Needs hipcc, no GPU.

    python tools/isa_identity.py OLD NEW [--jobs 4] [--work DIR] [--rename OLD_SYMBOL=NEW_SYMBOL ...]

OLD and NEW are each a checkout (a directory holding ofdm_amd/build.py) or a git revision of this repository, which is
exported into the work directory.  Every entry of each tree's own SOURCES is compiled with its own FLAGS + EXTRA_FLAGS plus
--offload-device-only -S, once as is and once with -DOFDM_PROFILE_BUILD=1.  Compared per kernel:
  text        the lines from `.type NAME,@function` to the next `.Lfunc_endN:`, without comments, empty lines and the
              directives in DROP, local labels without their per-file function counter (it moves when a file is split)
  descriptor  the lines between `.amdhsa_kernel NAME` and `.end_amdhsa_kernel`
Exit status 0 only if both trees have the same set of kernel names and every kernel's text and descriptor are equal.
With --work the .s files are kept there and reused while they are newer than csrc/.  --rename (repeatable, mangled names) says
that a kernel of OLD has another name in NEW: it is compared under the new name, with its own old name replaced in its text and
descriptor; without it such a kernel is reported once as "only in old" and once as "only in new".
"""
import argparse
import os
import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = re.compile(r"\s*\.(p2align|globl|protected|weak|hidden|section|text)\b")


def kernels(path):
    """{name: (text lines, descriptor lines)} of every kernel (a function with an .amdhsa_kernel block) in one .s"""
    text, desc, name, dname = {}, {}, None, None
    for line in open(path, errors="replace"):
        s = line.split(";")[0].rstrip()
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        d = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if d:  # the descriptor sits inside the function's range (a .rodata island before .Lfunc_end), so it is in the text too
            dname, desc[d.group(1)] = d.group(1), []
        elif dname and ".end_amdhsa_kernel" in line:
            dname = None
        elif dname:
            desc[dname].append(s.strip())
        if m:
            name, text[m.group(1)] = m.group(1), []
        elif name and re.match(r"\s*\.Lfunc_end\d+:", line):
            name = None
        elif name and s.strip() and not DROP.match(s):
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            text[name].append(re.sub(r"\.L(tmp|func_begin|JTI)\d+", r".L\1", s))
    return {k: (text.get(k), desc[k]) for k in desc}


def tree_of(spec, work, tag):
    if os.path.exists(os.path.join(spec, "ofdm_amd", "build.py")):
        return os.path.abspath(spec)
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--verify", spec + "^{commit}"], text=True).strip()
    dst = os.path.join(work, f"{tag}_{rev[:12]}")
    if not os.path.isdir(dst):
        os.makedirs(dst)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "ofdm_amd/build.py", "ofdm_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", dst], stdin=tar.stdout)
    return dst


def compile_tree(tree, out, jobs):
    """-> {(build, source file): {kernel: (text, descriptor)}} for build in ("plain", "profile")"""
    b = runpy.run_path(os.path.join(tree, "ofdm_amd", "build.py"))
    csrc = os.path.join(tree, "ofdm_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".h")))
    todo = []
    for build, define in (("plain", []), ("profile", ["-DOFDM_PROFILE_BUILD=1"])):
        for s in b["SOURCES"]:
            asm = os.path.join(out, build, s.replace(".hip", ".s"))
            os.makedirs(os.path.dirname(asm), exist_ok=True)
            cmd = [b["_hipcc"](), *b["FLAGS"], *define, *b["EXTRA_FLAGS"].get(s, []), "--offload-device-only", "-S", os.path.join(csrc, s), "-o", asm]
            todo.append((build, s, asm, None if os.path.exists(asm) and os.path.getmtime(asm) > newest else cmd))

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stderr)

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(run, [t[3] for t in todo if t[3]]))
    return {(build, s): kernels(asm) for build, s, asm, _ in todo}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--work", help="keep exported trees and .s files here (default: a temporary directory)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD_SYMBOL=NEW_SYMBOL", help="a kernel of OLD is NEW_SYMBOL in NEW")
    a = ap.parse_args()
    rename = dict(r.split("=", 1) for r in a.rename)
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = os.path.abspath(a.work or tmp.name)
    os.makedirs(work, exist_ok=True)
    old = compile_tree(tree_of(a.old, work, "old"), os.path.join(work, "old_s"), a.jobs)
    new = compile_tree(tree_of(a.new, work, "new"), os.path.join(work, "new_s"), a.jobs)
    for ks in old.values():
        for k in [k for k in ks if k in rename]:
            text, desc = ks.pop(k)
            ks[rename[k]] = ([s.replace(k, rename[k]) for s in text], [s.replace(k, rename[k]) for s in desc])
    print(subprocess.check_output(["hipcc", "--version"], text=True).splitlines()[0])
    for k, v in rename.items():
        print(f"renamed: `{k}` -> `{v}`")
    print("| build | source file (new tree) | kernels | identical | different |\n|---|---|---|---|---|")
    bad = []
    for build in ("plain", "profile"):
        was = {k: v for (b, _), ks in old.items() if b == build for k, v in ks.items()}
        now = {k: v for (b, _), ks in new.items() if b == build for k, v in ks.items()}
        for (b, s), ks in new.items():
            if b == build and ks:
                diff = sorted(k for k in ks if k in was and was[k] != ks[k])
                bad += [f"{build} {s}: differs: {k}" for k in diff]
                print(f"| {build} | {s} | {len(ks)} | {sum(1 for k in ks if was.get(k) == ks[k])} | {len(diff)} |")
        bad += [f"{build}: only in old: {k}" for k in sorted(set(was) - set(now))] + [f"{build}: only in new: {k}" for k in sorted(set(now) - set(was))]
        print(f"| {build} | all | {len(now)} (old tree: {len(was)}) | {sum(1 for k in now if was.get(k) == now[k])} | {sum(1 for k in now if k in was and was[k] != now[k])} |")
    print("\n".join(bad) if bad else "same kernel set, every kernel's text and descriptor equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
