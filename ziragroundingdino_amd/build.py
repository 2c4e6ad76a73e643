"""In-tree build of the HIP extension (``libzira_msda.so``) for gfx950.

``hipcc`` cross-compiles without a GPU; the shared object is written next to this file so it
travels with the tree (it is git-ignored, not gpurun-ignored).  Every source is compiled to its own
object under ``csrc/_obj`` (only what changed, a few at a time) and the objects are linked.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libzira_msda.so")
OBJ_DIR = os.path.join(_HERE, "csrc", "_obj")
SOURCES = [os.path.join(_HERE, "csrc", f) for f in ("msda.hip", "msda_cells.hip", "msda_tiles.hip", "msda_cpu.cpp", "rsb.hip", "rsb_ml.hip", "xty.hip", "xty_bf16x3.hip", "bisoftmax.hip", "layernorm.hip", "groupnorm.hip", "lsap.hip", "catlogits.hip", "winattn.hip", "refpoints.hip", "attn.hip", "sampling.hip", "gemm_drelu.hip", "rowgemm.hip", "gemm_bf16x3.hip", "gemm_f16x2.hip", "gemm_f16x2_panel.hip", "ffn_f16x2.hip", "thin_f16x2.hip", "criterion.hip", "textside.hip", "topk.hip", "grounding.hip", "optim_tail.hip", "ema.hip", "place.hip", "apmatch.hip", "resample.hip", "vocmatch.hip", "apaccum.hip", "metrics.hip", "nms.hip", "vocab.hip", "lvismatch.hip", "phrasematch.hip", "adapter.hip", "clslinear.hip", "prompt.hip", "prompt_memory.hip", "cet.hip", "lora.hip")]
HEADERS = [os.path.join(_ROOT, "include", "zira_msda.h"), os.path.join(_ROOT, "include", "zira_metrics.h"),
           os.path.join(_ROOT, "include", "zira_rsb_ml.h"), os.path.join(_ROOT, "include", "zira_nms.h"),
           os.path.join(_ROOT, "include", "zira_vocab.h"), os.path.join(_ROOT, "include", "zira_lvis.h"),
           os.path.join(_ROOT, "include", "zira_phrase.h"), os.path.join(_ROOT, "include", "zira_adapter.h"),
           os.path.join(_ROOT, "include", "zira_clslinear.h"), os.path.join(_ROOT, "include", "zira_prompt.h"),
           os.path.join(_ROOT, "include", "zira_prompt_memory.h"), os.path.join(_ROOT, "include", "zira_cet.h"),
           os.path.join(_ROOT, "include", "zira_lora.h"),
           os.path.join(_HERE, "csrc", "cat_max.h"), os.path.join(_HERE, "csrc", "prompt_table.h"),
           os.path.join(_HERE, "csrc", "msda_internal.h"),
           os.path.join(_HERE, "csrc", "msda_fwd_lean.h"), os.path.join(_HERE, "csrc", "split_arith.h"),
           os.path.join(_HERE, "csrc", "lane_sum.h"), os.path.join(_HERE, "csrc", "launch.h"),
           os.path.join(_HERE, "csrc", "mfma_f32_tile.h"), os.path.join(_HERE, "csrc", "ticket.h"),
           os.path.join(_HERE, "csrc", "gate.h"), os.path.join(_HERE, "csrc", "zero_loss.h"),
           os.path.join(_HERE, "csrc", "stable_desc.h"), os.path.join(_HERE, "csrc", "topk_select.h")]
HIPCC_FLAGS = [
    "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC",
    "-munsafe-fp-atomics",       # fp32 atomics -> global_atomic_add_f32 (no CAS loop)
    "-I" + os.path.join(_ROOT, "include"), "-pthread",
]
# per-source additions
EXTRA_FLAGS = {
    # packed fp32 vector instructions beside matrix instructions cost more than the two plain ones they replace
    "ffn_f16x2.hip": ["-fno-slp-vectorize"],
    # the canvas holds the bits of torch's `(x - mean) / std`: the divide stays the correctly rounded one, whatever the default
    "place.hip": ["-fhip-fp32-correctly-rounded-divide-sqrt"],
    # COCOeval's IoU is numpy / C doubles, every operation rounded on its own: `da + ga - w * h` must not become an FMA
    "apmatch.hip": ["-ffp-contract=off"],
    # COCOeval's precision is numpy doubles too: `tp + fp + eps` stays an add in front of the divide
    "apaccum.hip": ["-ffp-contract=off"],
    # voc_eval's overlap is numpy doubles too, and so is the text round trip of the detections that the kernel restates
    "vocmatch.hip": ["-ffp-contract=off"],
    # Pillow's resampling coefficients are C doubles, every operation rounded on its own: `(xx + 0.5) * scale - support` stays two
    "resample.hip": ["-ffp-contract=off"],
    # the metrics log's rank means, totals, medians and window means are numpy doubles, bit for bit: `0.0 + sum` and the
    # pairwise sums stay the additions they are written as
    "metrics.hip": ["-ffp-contract=off"],
    # the NMS's IoU is torch's fp32 arithmetic, every operation rounded on its own and the divide the correctly rounded one:
    # `area_i + area_j - inter` must not become an FMA, and a pair that sits exactly on the threshold has to stay there
    "nms.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # the merged tail's box arithmetic is the detections tail's: topk.hip is built with no flag of its own and spells the chain
    # with the rounding intrinsics under `fp contract(off)` (topk_select.h, shared); the flag here only says the same once more
    "vocab.hip": ["-ffp-contract=off"],
    # LVISEval's IoU is numpy doubles as COCOeval's is: `da + ga - w * h` must not become an FMA
    "lvismatch.hip": ["-ffp-contract=off"],
    # the phrase matching's IoU is fp64 with every operation rounded on its own, as the three box evaluators' is
    "phrasematch.hip": ["-ffp-contract=off"],
    # the adapter's gate divides by two norms and takes their roots once per row: the correctly rounded ones, as the op chain's
    "adapter.hip": ["-fhip-fp32-correctly-rounded-divide-sqrt"],
    # the CET adapter's gate is the same expression over the text encoder's states
    "cet.hip": ["-fhip-fp32-correctly-rounded-divide-sqrt"],
}
JOBS = 4


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found; the HIP extension cannot be built")
    return exe


def _obj(src):
    return os.path.join(OBJ_DIR, os.path.basename(src) + ".o")


def _stale(src, newest_common):
    o = _obj(src)
    return not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(src), newest_common)


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS + [__file__])


def build_extension(force=False, verbose=False):
    """Compile every HIP source into libzira_msda.so (no-op when up to date)."""
    if not force and not needs_build():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    common = max(os.path.getmtime(p) for p in HEADERS + [__file__])
    hipcc = _hipcc()

    def compile_one(src):
        cmd = [hipcc] + HIPCC_FLAGS + EXTRA_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", _obj(src) + ".tmp"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(_obj(src) + ".tmp", _obj(src))

    todo = [s for s in SOURCES if force or _stale(s, common)]
    with ThreadPoolExecutor(max_workers=JOBS) as pool:
        list(pool.map(compile_one, todo))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + [_obj(s) for s in SOURCES] + ["-o", LIB_PATH + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_extension(force=True, verbose=True))
