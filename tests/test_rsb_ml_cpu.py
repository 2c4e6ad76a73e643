"""The multilayer-branch epilogue without a GPU: its C ABI is declared in include/zira_rsb_ml.h, typed from that header and
exported by the built library, and CPU tensors never reach it, whatever the switch says."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import rsb_multilayer as ml

ENTRIES = ["zira_rsb_l1_workspace_floats", "zira_rsb_l1_fwd_f32", "zira_rsb_l1_bwd_f32",
           "zira_rsb_gn_workspace_floats", "zira_rsb_gn_fwd_f32", "zira_rsb_gn_bwd_f32"]


def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_rsb_ml.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.RSB_ML_SYMBOLS)
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    P = _lib.RSB_ML_PROTOTYPES
    assert P["zira_rsb_l1_workspace_floats"] == (sz, [sz])
    assert P["zira_rsb_l1_fwd_f32"] == (i, [vp, vp, vp, sz, vp, vp, vp, vp])
    assert P["zira_rsb_l1_bwd_f32"] == (i, [vp] * 5 + [sz] + [vp] * 5)
    assert P["zira_rsb_gn_workspace_floats"] == (sz, [i] * 4)
    assert P["zira_rsb_gn_fwd_f32"] == (i, [vp] * 5 + [i] * 4 + [f32] + [vp] * 6)
    assert P["zira_rsb_gn_bwd_f32"] == (i, [vp] * 9 + [i] * 4 + [vp] * 7)
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert not set(ENTRIES) & set(_lib.SYMBOLS)        # zira_msda.h's own surface is what it was


def test_host_side_answers():
    lib = _lib.load()
    assert lib.zira_rsb_l1_workspace_floats(1) > 0 and lib.zira_rsb_l1_workspace_floats(0) == 0
    # the model's levels (B = 2, C = 256, G = 32): the first is split 4 ways, 10 floats of scratch per block
    assert lib.zira_rsb_gn_workspace_floats(2, 256, 100 * 167, 32) == 2 * 256 * 4 * 10
    assert lib.zira_rsb_gn_workspace_floats(2, 256, 13 * 21, 32) == 2 * 256 * 10
    assert lib.zira_rsb_gn_workspace_floats(1, 32, 1, 32) == 32 * 10
    for bad in ((2, 48, 35, 32), (0, 32, 4, 32), (2, 32, 0, 32), (2, 32, 4, 0), (1 << 12, 1 << 12, 4, 32), (1, 32, (1 << 28) + 1, 32)):
        assert lib.zira_rsb_gn_workspace_floats(*bad) == 0, bad
    # declined arguments are reported and nothing is launched
    assert lib.zira_rsb_gn_fwd_f32(None, None, None, None, None, 2, 256, 35, 32, 1e-5, None, None, None, None, None, None) == -1
    assert lib.zira_rsb_l1_bwd_f32(None, None, None, None, None, 4, None, None, None, None, None) == -1


def _forward_backward(mod, x):
    mod.train()
    x = x.clone().requires_grad_(True)
    out, zl = mod(x)
    grads = torch.autograd.grad(out.square().sum() + 0.3 * zl, [x] + list(mod.parameters()))
    mod.eval()
    return [out.detach(), zl.detach()] + list(grads) + [t.detach() for t in mod(x)]


@pytest.mark.parametrize("kind", ["conv1x1", "conv3x3s2", "linear"])
def test_cpu_tensors_ignore_the_switch(monkeypatch, kind):
    assert ml.NATIVE_EPILOGUE is False          # nothing turns it on by default
    torch.manual_seed(11)
    if kind == "linear":
        mod, x = ml.RepZeroLinear(24, 16), torch.randn(2, 5, 24)
    else:
        kw = dict(kernel_size=1) if kind == "conv1x1" else dict(kernel_size=3, stride=2, padding=1)
        mod, x = ml.RepZeroConv2dGN(12, 64, **kw), torch.randn(2, 12, 7, 9)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    off = _forward_backward(mod, x)
    monkeypatch.setattr(ml, "NATIVE_EPILOGUE", True)
    on = _forward_backward(mod, x)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
