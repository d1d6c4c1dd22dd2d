#!/usr/bin/env python3
"""One line per kernel of a source file, as csrc/Makefile builds it: hipcc's
-Rpass-analysis=kernel-resource-usage figures and instruction counts from the device assembly.

usage: tools/kernel_resources.py physicsbasedbayesianinference_amd/csrc/kernels_dense.hip [extra hipcc flags]

The per-file switches (FLAGS_<name> of csrc/Makefile) are taken from the Makefile of the source's directory.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hipcc_asm import device_asm_command  # noqa: E402

src = sys.argv[1]
stem = os.path.splitext(os.path.basename(src))[0]
with tempfile.TemporaryDirectory() as tmp:
    asm = os.path.join(tmp, stem + ".s")
    cmd = device_asm_command(src, asm, ["-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:])
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    text = open(asm).read() if os.path.exists(asm) else ""
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"remark: [^:]+:\d+:\d+:\s+(.*?)\s*\[-Rpass", line) or re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
    if not m:
        if "error" in line:
            print(line)
        continue
    txt = m.group(1)
    if txt.startswith("Function Name:"):
        cur = {"name": txt.split(":", 1)[1].strip()}
        rows.append(cur)
    elif cur is not None and ":" in txt:
        k, v = txt.split(":", 1)
        cur[k.strip()] = v.strip()
# instructions of each kernel: from its label to its .Lfunc_end
COUNTED = [("f64", r"v_\w+_f64"), ("bld", r"buffer_load\w*"), ("bst", r"buffer_store\w*"), ("glob", r"global_\w+"),
           ("ds", r"ds_\w+"), ("barr", r"s_barrier"), ("wait", r"s_waitcnt")]
for r in rows:
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(r["name"]), text, re.S | re.M)
    ops = [ln.split()[0] for ln in (m.group(1).splitlines() if m else []) if ln.startswith("\t") and not ln.startswith("\t.")]
    for key, pat in COUNTED:
        r[key] = sum(1 for op in ops if re.fullmatch(pat, op)) if m else "?"
keys = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
        "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"] + [k for k, _ in COUNTED]
fmt = "%-70s %5s %5s %5s %7s %3s %6s %6s %6s" + " %5s" * len(COUNTED)
print(fmt % tuple(["kernel", "VGPR", "AGPR", "SGPR", "scratch", "occ", "sSpill", "vSpill", "LDS"] + [k for k, _ in COUNTED]))
for r in rows:
    name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*\)$", "", name)[:70]  # the parameter list (struct names) says nothing the template arguments do not
    print(fmt % tuple([name] + [r.get(k, "?") for k in keys]))
