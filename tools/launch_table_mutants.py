#!/usr/bin/env python3
"""tools/launch_table_mutants.py -- does tests/data/launch_table.txt see every rule of csrc/csic_select.cpp?  Flips every comparison
and logical operator and nudges every integer constant (+1, -1, x2, /2) in the code lines of selection and geometry (not the
name formatting, not fill_base_args), builds tests/cpp/launch_table.cpp against each mutant (g++, CPU only, about two minutes on
24 threads) and sorts the mutants into
  killed      a line of the committed table moves, or an invariant of the program breaks;
  SURVIVED    the committed table does not move although the whole cross product (launch_table --full) does: add a case;
  unseen      neither moves: the mutant is equivalent on the parameter domain (factors 1 / 2 / 4 / 8, holds 1 / 2 / 4, ...) or
              sits in a value nothing reads; each one is listed for a reader to judge (profiles/r07_planner_refactor.md does, and
              profiles/r17_planner_planes.md for the plane units' planning functions)."""
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ROOT + "/chroma-subsampling-image-compressor_amd/csrc"
SRC = CSRC + "/csic_select.cpp"
WORK = tempfile.mkdtemp(prefix="launch_table_mutants_")
FIX = open(ROOT + "/tests/data/launch_table.txt").read()

lines = open(SRC).read().split("\n")
OPS = [("<=", "<"), (">=", ">"), ("==", "!="), ("!=", "=="), ("&&", "||"), ("||", "&&"), ("<", "<="), (">", ">=")]
tok = re.compile(r"<=|>=|==|!=|&&|\|\||<<|>>|->|<|>|\b\d+\b")


def code_part(l):
    i = l.find("//")
    return l if i < 0 else l[:i]


start = next(i for i, l in enumerate(lines) if l.startswith("static int dec_block_x"))
skip_fn = False
mutants = []
for i in range(start, len(lines)):
    l = lines[i]
    if l.startswith("void fill_base_args") or re.match(r"void \w*kernel_name\(", l):        # every name function, the plane units' too
        skip_fn = True
    elif skip_fn and l.startswith("}"):
        skip_fn = False
        continue
    if skip_fn:
        continue
    c = code_part(l)
    if "set_error" in c or "snprintf" in c or c.strip().startswith('"') or "#include" in c or "template" in c:
        continue
    for m in tok.finditer(c):
        t = m.group(0)
        reps = []
        if t in ("<<", ">>", "->"):
            continue
        if t.isdigit():
            v = int(t)
            reps = [str(v + 1)] + ([str(v - 1)] if v > 0 else [])
            if v >= 8:
                reps += [str(v * 2), str(v // 2)]
        else:
            if t in ("<", ">") and re.search(r"(static_cast|Dim3|uint32_t|int64_t|int32_t)\s*$", c[:m.start()]):
                continue
            reps = [b for a, b in OPS if a == t]
        for r in reps:
            new = c[:m.start()] + r + c[m.end():] + l[len(c):]
            mutants.append((i, m.start(), t, r, new))

base_objs = None


def run(idx):
    i, col, t, r, new = mutants[idx]
    src = f"{WORK}/m{idx}.cpp"
    exe = f"{WORK}/m{idx}"
    body = lines[:i] + [new] + lines[i + 1:]
    open(src, "w").write("\n".join(body))
    cp = subprocess.run(["g++", "-std=c++17", "-O0", "-w", "-I" + ROOT + "/include", "-I" + CSRC, "-c", src, "-o", exe + ".o"], capture_output=True)
    if cp.returncode:
        return idx, "nocompile", ""
    subprocess.check_call(["g++", exe + ".o", WORK + "/lt.o", WORK + "/host.o", "-o", exe])
    try:
        a = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        return idx, "killed(timeout)", ""
    if a.returncode != 0 or a.stdout != FIX:
        res = "killed"
    else:
        try:
            b = subprocess.run([exe, "--full"], capture_output=True, timeout=120)
            h = hashlib.md5(b.stdout).hexdigest()
            res = "SURVIVED" if (h != FULL or b.returncode != 0) else "unseen"
        except subprocess.TimeoutExpired:
            res = "SURVIVED(timeout in full)"
    for f in (src, exe, exe + ".o"):
        if os.path.exists(f):
            os.remove(f)
    return idx, res, ""


subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + ROOT + "/include", "-I" + CSRC, "-c", ROOT + "/tests/cpp/launch_table.cpp", "-o", WORK + "/lt.o"])
subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + ROOT + "/include", "-I" + CSRC, "-c", CSRC + "/csic_host.cpp", "-o", WORK + "/host.o"])
subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + ROOT + "/include", "-I" + CSRC, "-c", SRC, "-o", WORK + "/sel.o"])
subprocess.check_call(["g++", WORK + "/sel.o", WORK + "/lt.o", WORK + "/host.o", "-o", WORK + "/base"])
out = subprocess.run([WORK + "/base"], capture_output=True, text=True).stdout
assert out == FIX, "the unmutated planner does not reproduce the fixture"
FULL = hashlib.md5(subprocess.run([WORK + "/base", "--full"], capture_output=True).stdout).hexdigest()

import shutil
counts = {}
surv = []
with cf.ThreadPoolExecutor(int(os.environ.get("JOBS", "24"))) as ex:
    for idx, res, _ in ex.map(run, range(len(mutants))):
        counts[res] = counts.get(res, 0) + 1
        if res.startswith("SURVIVED") or res == "unseen":
            i, col, t, r, new = mutants[idx]
            surv.append((res, i + 1, t, r, new.strip()[:150]))
shutil.rmtree(WORK, ignore_errors=True)
print(len(mutants), "mutants:", counts)
for s in sorted(surv):
    print(*s, sep=" | ")
