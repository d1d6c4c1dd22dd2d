#!/usr/bin/env python3
"""Instruction counts per loop nest of the kernels of one source file, as csrc/Makefile builds it.

usage: tools/loop_valu_count.py physicsbasedbayesianinference_amd/csrc/kernels_dense.hip 'k_dense_hmc<8, true, 0, true, 0, false, 2, true, 0' [--top 8] [--asm kept.s] [extra hipcc flags]

The source is compiled to device assembly with the per-file switches of the Makefile next to it (FLAGS_<name>, like
tools/kernel_resources.py).  Every kernel whose demangled name contains the pattern is cut into its loops, as the
compiler's own block comments name them ("in Loop: Header=", "Parent Loop"), so that a block laid out behind the
loop's last branch still counts for its loop.  Per loop the report gives the
counts of MFMA, other vector ALU, LDS, vector memory, s_waitcnt and s_nop instructions -- once for the whole span
(one trip of the loop with one trip of everything inside it) and once for every stretch of the loop's own code
between its inner loops -- and the most frequent opcodes of each stretch.  Lane reads and writes (the reloads and
saves of scalars parked in vector lanes) are listed on their own.  A report, not a test: it says what a trip costs
in issue slots, not what it costs in time.  --asm reads an assembly file instead of compiling (and keeps nothing).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hipcc_asm import device_asm_command  # noqa: E402

CLASSES = [("mfma", r"v_mfma\w*"), ("valu", r"v_\w+"), ("lds", r"ds_\w+"),
           ("vmem", r"(buffer|global|flat|scratch)_\w+"), ("wait", r"s_waitcnt\w*"), ("nop", r"s_nop")]
LANE = r"v_(readlane|writelane)_b32"


def classify(op):
    for name, pat in CLASSES:
        if re.fullmatch(pat, op):
            return name
    return "salu" if op.startswith("s_") else "other"


def compile_asm(src, extra):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, os.path.splitext(os.path.basename(src))[0] + ".s")
        done = subprocess.run(device_asm_command(src, asm, extra), capture_output=True, text=True)
        if done.returncode != 0 or not os.path.exists(asm):
            sys.exit(done.stderr)
        return open(asm).read()


def kernels(text):
    """(mangled name, body lines) of every function of the assembly"""
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        yield m.group(1), m.group(2).splitlines()


def demangle(name):
    out = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    out = re.sub(r"\(anonymous namespace\)::", "", out)
    return re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", out))


def parse(lines):
    """instructions [(opcode, operands, loop)]: loop is the header label of the innermost loop the instruction's
    block belongs to (None outside loops), read from the comments LLVM puts on every block; and {loop: parent}"""
    ins, parent = [], {}
    cur, label = None, None
    for ln in lines:
        m = re.match(r"^\.L(BB\d+_\d+):", ln) or re.match(r"^; %bb\.\d+:", ln)
        if m:
            label = m.group(1) if m.lastindex else None
            cur = None  # until a loop comment on this or the following lines says otherwise
        note = ln.split(";", 1)[1] if ";" in ln else ""
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
        if m:
            cur = m.group(1)
        m = re.search(r"Parent Loop (BB\d+_\d+)", note)
        if m and label:
            parent[label] = m.group(1)  # the last "Parent Loop" line names the innermost parent
        if re.search(r"This (Inner )?Loop Header", note) and label:
            cur = label
            parent.setdefault(label, None)
        if not ln.startswith("\t") or ln.startswith("\t.") or ln.startswith("\t;"):
            continue
        parts = ln.split(";")[0].split(None, 1)
        if parts:
            ins.append((parts[0], parts[1].strip() if len(parts) > 1 else "", cur))
    return ins, parent


def summary(chunk, top):
    cnt = collections.Counter(classify(i[0]) for i in chunk)
    lane = sum(1 for i in chunk if re.fullmatch(LANE, i[0]))
    ops = collections.Counter(i[0] for i in chunk if classify(i[0]) in ("valu", "salu"))
    head = "mfma %4d  valu %4d  lds %4d  vmem %4d  s_waitcnt %3d  s_nop %3d  lane r/w %3d" % (
        cnt["mfma"], cnt["valu"], cnt["lds"], cnt["vmem"], cnt["wait"], cnt["nop"], lane)
    return head, ", ".join("%s %d" % kv for kv in ops.most_common(top))


def report(name, lines, top):
    ins, parent = parse(lines)
    print("%s\n  %d instructions, %d loops" % (name, len(ins), len(parent)))
    print("  whole kernel:  %s" % summary(ins, top)[0])

    def inside(loop, of):  # is `loop` the loop `of` or nested in it
        while loop is not None and loop != of:
            loop = parent.get(loop)
        return loop == of

    def walk(loop, depth, tag):
        pad = "  " * (depth + 1)
        body = [i for i in ins if inside(i[2], loop)]
        print("%sloop %s (.L%s) [%d instructions]\n%s  one trip, inner loops once:  %s"
              % (pad, tag, loop, len(body), pad, summary(body, top)[0]))
        # the loop's own code in layout order, cut where an inner loop (or code outside the loop) stands between
        stretches, kids, run = [], [], []
        for i in ins:
            if i[2] == loop:
                run.append(i)
                continue
            if run:
                stretches.append(run)
                run = []
            if inside(i[2], loop):
                kid = i[2]
                while parent.get(kid) != loop:
                    kid = parent[kid]
                if kid not in kids:
                    kids.append(kid)
                    stretches.append(kid)
        if run:
            stretches.append(run)
        n = k = 0
        for st in stretches:
            if isinstance(st, str):
                k += 1
                walk(st, depth + 1, "%s.%d" % (tag, k))
            elif len(st):
                n += 1
                head, ops = summary(st, top)
                print("%s  own code, stretch %d:  %s\n%s    most frequent: %s" % (pad, n, head, pad, ops))

    for n, loop in enumerate(l for l in parent if parent[l] is None):
        walk(loop, 0, str(n + 1))
    print()


def main():
    args = sys.argv[1:]
    top, asm = 8, None
    for flag in ("--top", "--asm"):
        if flag in args:
            i = args.index(flag)
            val = args[i + 1]
            del args[i:i + 2]
            if flag == "--top":
                top = int(val)
            else:
                asm = val
    if len(args) < 2:
        sys.exit(__doc__)
    src, pattern, extra = args[0], args[1], args[2:]
    text = open(asm).read() if asm else compile_asm(src, extra)
    found = 0
    for mangled, lines in kernels(text):
        name = demangle(mangled)
        if pattern in name:
            report(name, lines, top)
            found += 1
    if not found:
        sys.exit("no kernel of %s matches %r" % (src, pattern))


if __name__ == "__main__":
    main()
