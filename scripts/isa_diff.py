"""Kernel-by-kernel comparison of the gfx950 machine code of every device source in two trees (CPU only).

    python scripts/isa_diff.py BEFORE_ROOT [AFTER_ROOT] [--out FILE]

The sources are the union of build.SOURCES of both trees, .cpp files skipped.  For each source of each tree: the device
object is built with the flags of ziragroundingdino_amd/build.py plus --cuda-device-only -c, unbundled for gfx950,
disassembled without addresses or raw bytes, stripped of `//` comments and cut into kernels.  Prints one line per kernel
(identical / DIFFERENT / only before / only after) and exits 1 when a kernel present in both trees differs.  A source
missing from one tree lists its kernels as only in the other.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def build_module(root):
    spec = importlib.util.spec_from_file_location("_zira_build", os.path.join(root, "ziragroundingdino_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_sources(mod):
    return [os.path.basename(s) for s in mod.SOURCES if not s.endswith(".cpp")]


def kernels(root, mod, src, tmp, label):
    path = os.path.join(root, "ziragroundingdino_amd", "csrc", src)
    if not os.path.exists(path) or src not in device_sources(mod):
        return {}
    tag = os.path.join(tmp, "%s_%s" % (label, src))
    subprocess.check_call([mod._hipcc()] + mod.HIPCC_FLAGS + mod.EXTRA_FLAGS.get(src, []) +
                          ["--cuda-device-only", "-c", path, "-o", tag + ".bundle"])
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
        if line == "...":        # objdump's mark for zero padding behind a symbol: it depends on what follows, not on the kernel
            continue
        if name is not None and line:
            out[name].append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    roots = {"before": os.path.abspath(a.before), "after": os.path.abspath(a.after)}
    mods = {k: build_module(r) for k, r in roots.items()}
    sources = device_sources(mods["before"])
    sources += [s for s in device_sources(mods["after"]) if s not in sources]
    lines, differ = ["# gfx950 device code of every device source in build.SOURCES, kernel by kernel: the BEFORE tree against the "
                     "AFTER tree (hipcc flags of build.py + --cuda-device-only -c; llvm-objdump without addresses, raw bytes or "
                     "comments)"], 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.jobs) as pool:
        jobs = {(src, k): pool.submit(kernels, roots[k], mods[k], src, tmp, k) for src in sources for k in roots}
        width = max(len(s) for s in sources) + 1
        for src in sources:
            kb, ka = jobs[(src, "before")].result(), jobs[(src, "after")].result()
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
                lines.append("%-*s %-30s %s" % (width, src, state, name))
    lines.append("%d kernel(s) present in both trees differ" % differ)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
