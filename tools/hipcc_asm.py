"""The hipcc line that compiles one source of csrc/ to device assembly the way csrc/Makefile builds it: the common
flags plus the per-file switches (FLAGS_<name>), which are asked of the Makefile next to the source
(make print-flags-<name>).  Shared by tools/kernel_resources.py and tools/loop_valu_count.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm_command(src, asm, extra=()):
    src_dir = os.path.dirname(os.path.abspath(src))
    stem = os.path.splitext(os.path.basename(src))[0]
    made = subprocess.run(["make", "-s", "-C", src_dir, "print-flags-" + stem], capture_output=True, text=True)
    if made.returncode != 0:
        sys.exit("csrc/Makefile has no print-flags-%% target: %s" % made.stderr.strip())
    return ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "include"), "-I" + src_dir] + made.stdout.split() + \
           ["--cuda-device-only", "-S", src, "-o", asm] + list(extra)
