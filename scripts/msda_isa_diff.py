"""Kernel-by-kernel comparison of the gfx950 machine code of the MSDA sources in two trees (CPU only).

    python scripts/msda_isa_diff.py BEFORE_ROOT [AFTER_ROOT] [--out FILE]

For msda.hip, msda_cells.hip and msda_tiles.hip of each tree: the device object is built with the flags of
ziragroundingdino_amd/build.py plus --cuda-device-only -c, unbundled for gfx950, disassembled without addresses or
raw bytes, stripped of `//` comments and cut into kernels.  Prints one line per kernel (identical / DIFFERENT /
only before / only after) and exits 1 when a kernel present in both trees differs.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

SOURCES = ("msda.hip", "msda_cells.hip", "msda_tiles.hip")
LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def build_flags(root):
    spec = importlib.util.spec_from_file_location("_zira_build", os.path.join(root, "ziragroundingdino_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._hipcc(), mod.HIPCC_FLAGS, mod.EXTRA_FLAGS


def kernels(root, src, tmp, label):
    hipcc, flags, extra = build_flags(root)
    path = os.path.join(root, "ziragroundingdino_amd", "csrc", src)
    tag = os.path.join(tmp, "%s_%s" % (label, src))
    subprocess.check_call([hipcc] + flags + extra.get(src, []) + ["--cuda-device-only", "-c", path, "-o", tag + ".bundle"])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + tag + ".bundle", "--output=" + tag + ".o"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                    "--demangle", tag + ".o"], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        line = line.split("//")[0].strip()
        if name is not None and line:
            out[name].append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    a = ap.parse_args()
    lines, differ = ["# gfx950 device code of %s, kernel by kernel: the BEFORE tree against the AFTER tree (hipcc flags of build.py "
                     "+ --cuda-device-only -c; llvm-objdump without addresses, raw bytes or comments)" % ", ".join(SOURCES)], 0
    with tempfile.TemporaryDirectory() as tmp:
        for src in SOURCES:
            kb, ka = kernels(os.path.abspath(a.before), src, tmp, "before"), kernels(os.path.abspath(a.after), src, tmp, "after")
            for name in sorted(set(kb) | set(ka)):
                if name not in ka:
                    state = "only before"
                elif name not in kb:
                    state = "only after"
                elif kb[name] == ka[name]:
                    state = "identical (%d instructions)" % len(ka[name])
                else:
                    state = "DIFFERENT"
                    differ += 1
                lines.append("%-15s %-30s %s" % (src, state, name))
    lines.append("%d kernel(s) present in both trees differ" % differ)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
