"""The fused epilogue of the multilayer-branch side branches (csrc/rsb_ml.hip, include/zira_rsb_ml.h) on the MI355X.

Oracle: the defining expression in float64 with torch ops and autograd on the same device.  Yardstick: the float32 op chain on
the same inputs -- what ``rsb_multilayer`` runs with ``NATIVE_EPILOGUE`` off.  For every output and every gradient

    max|kernel - fp64|  <=  2 * max|op chain - fp64|  +  one fp32 ulp of the tensor's largest magnitude

both errors measured here, nothing fixed in advance: the factor 2 covers a different but equally valid order of summation,
the ulp a tensor the op chain happens to get exactly right.  Every figure is printed before it is asserted (``pytest -s``).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import rsb_multilayer as ml

pytestmark = pytest.mark.gpu

G, EPS = 32, 1e-5
GN_SHAPES = [(1, 32, 1), (2, 256, 35), (2, 256, 221), (1, 256, 16700), (3, 64, 50)]
L1_SIZES = [1, 12345, 2 * 195 * 256]
REGIMES = ["o1", "zira"]
GRAD_LOSS = 0.37


def dev():
    return torch.device("cuda:0")


def ulp(t):
    return float(np.spacing(np.float32(float(t.detach().abs().max()))))


def within_bar(what, kernel, chain, ref, sel=None):
    """The bar of the module docstring; `sel` restricts the kernel's error to some positions (the bar stays the tensor's)."""
    kernel, chain, ref = kernel.detach().double().reshape(-1), chain.detach().double().reshape(-1), ref.detach().reshape(-1)
    assert torch.isfinite(kernel).all(), what
    err_c = float((chain - ref).abs().max())
    dk = (kernel - ref).abs()
    err_k = float((dk if sel is None else dk[sel]).max())
    bar = 2.0 * err_c + ulp(ref)
    print("%-28s kernel %.3e  chain %.3e  bar %.3e  (max|ref| %.3e)" % (what, err_k, err_c, bar, float(ref.abs().max())))
    assert err_k <= bar, "%s: kernel %.3e > bar %.3e (chain %.3e)" % (what, err_k, bar, err_c)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _inputs(shape, regime, seed, vision):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    C = shape[1] if vision else 1
    if regime == "o1":
        d = dict(yb=r(*shape), yt=r(*shape) * 1.5 + 3.0, s=torch.tensor([0.7]), gamma=r(C), beta=r(C))
    else:       # the ZiRa regime: a 1e-8 branch on an O(1) twin, the affine parameters as ZeroGroupNorm starts them
        d = dict(yb=r(*shape) * 1e-8, yt=r(*shape) * 1.5 + 3.0, s=torch.ones(1), gamma=torch.full((C,), 1e-8),
                 beta=torch.full((C,), 1e-8))
    d["go"] = r(*shape)
    d["gl"] = torch.tensor(GRAD_LOSS)
    if not vision:
        del d["gamma"], d["beta"]
    return {k: v.to(dev()) for k, v in d.items()}


def gn_chain(yb, yt, s, gamma, beta):
    """today's RepZeroConv2dGN.forward behind the two convolutions; native_group_norm is what F.group_norm calls and also
    returns the statistics"""
    B, C, HW = yb.shape
    branch = yb * s
    out, mean, rstd = torch.native_group_norm(branch + yt, gamma, beta, B, C, HW, G, EPS)
    return out, branch.abs().mean() + out.abs().mean(), mean.reshape(-1), rstd.reshape(-1)


def l1_chain(yb, yt, s):
    branch = s * yb
    out = branch + yt
    return out, branch.abs().mean() + out.abs().mean()


def chain_run(fn, leaves, go, gl, mode):
    """forward and the gradients of sum(out * go) + gl * loss (mode: both / no_go / no_gl / no_twin) for every leaf"""
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    res = fn(*leaves)
    obj = 0
    if mode != "no_go":
        obj = obj + (res[0] * go.to(res[0].dtype)).sum()
    if mode != "no_gl":
        obj = obj + gl.to(res[1].dtype) * res[1]
    return [t.detach() for t in res], list(torch.autograd.grad(obj, leaves))


@functools.lru_cache(maxsize=None)
def gn_case(shape, regime):
    """inputs, and per mode the fp64 oracle and the fp32 op chain; computed once, read by every test of the case"""
    d = _inputs(shape, regime, 100 + GN_SHAPES.index(shape) if shape in GN_SHAPES else 7, True)
    leaves = [d[k] for k in ("yb", "yt", "s", "gamma", "beta")]
    runs = {}
    for mode in ("both", "no_go", "no_gl"):
        runs[mode] = (chain_run(gn_chain, [t.double() for t in leaves], d["go"], d["gl"], mode),
                      chain_run(gn_chain, leaves, d["go"], d["gl"], mode))
    runs["no_twin"] = runs["both"]
    return d, runs


@functools.lru_cache(maxsize=None)
def l1_case(n, regime):
    d = _inputs((n,), regime, 200 + L1_SIZES.index(n), False)
    leaves = [d[k] for k in ("yb", "yt", "s")]
    runs = {mode: (chain_run(l1_chain, [t.double() for t in leaves], d["go"], d["gl"], mode),
                   chain_run(l1_chain, leaves, d["go"], d["gl"], mode)) for mode in ("both", "no_go", "no_gl")}
    return d, runs


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def native_gn_fwd(d):
    lib = _lib.load()
    B, C, HW = d["yb"].shape
    n_ws = lib.zira_rsb_gn_workspace_floats(B, C, HW, G)
    assert n_ws > 0
    ws = torch.empty(n_ws, device=dev())
    out, loss = torch.empty_like(d["yb"]), torch.empty(1, device=dev())
    mean, rstd = torch.empty(B * G, device=dev()), torch.empty(B * G, device=dev())
    rc = lib.zira_rsb_gn_fwd_f32(_p(d["yb"]), _p(d["yt"]), _p(d["s"]), _p(d["gamma"]), _p(d["beta"]), B, C, HW, G, EPS, _p(out),
                                 _p(loss), _p(mean), _p(rstd), _p(ws), _stream())
    assert rc == 0
    return out, loss[0], mean, rstd


def native_gn_bwd(d, fwd, mode):
    lib = _lib.load()
    B, C, HW = d["yb"].shape
    out, _, mean, rstd = fwd
    ws = torch.empty(lib.zira_rsb_gn_workspace_floats(B, C, HW, G), device=dev())
    gb = torch.empty_like(d["yb"])
    gt = torch.empty_like(d["yb"]) if mode != "no_twin" else None
    gs, gg, gbeta = torch.empty(1, device=dev()), torch.empty(C, device=dev()), torch.empty(C, device=dev())
    rc = lib.zira_rsb_gn_bwd_f32(_p(d["yb"]), _p(d["yt"]), _p(d["s"]), _p(d["gamma"]), _p(mean), _p(rstd), _p(out),
                                 _p(d["go"]) if mode != "no_go" else None, _p(d["gl"]) if mode != "no_gl" else None, B, C, HW, G,
                                 _p(gb), _p(gt), _p(gs), _p(gg), _p(gbeta), _p(ws), _stream())
    assert rc == 0
    return gb, gt, gs, gg, gbeta


def native_l1_fwd(d):
    lib = _lib.load()
    n = d["yb"].numel()
    ws = torch.empty(lib.zira_rsb_l1_workspace_floats(n), device=dev())
    out, loss = torch.empty_like(d["yb"]), torch.empty(1, device=dev())
    assert lib.zira_rsb_l1_fwd_f32(_p(d["yb"]), _p(d["yt"]), _p(d["s"]), n, _p(out), _p(loss), _p(ws), _stream()) == 0
    return out, loss[0]


def native_l1_bwd(d, mode):
    lib = _lib.load()
    n = d["yb"].numel()
    ws = torch.empty(lib.zira_rsb_l1_workspace_floats(n), device=dev())
    gb, gt, gs = torch.empty_like(d["yb"]), torch.empty_like(d["yb"]), torch.empty(1, device=dev())
    rc = lib.zira_rsb_l1_bwd_f32(_p(d["yb"]), _p(d["yt"]), _p(d["s"]), _p(d["go"]) if mode != "no_go" else None,
                                 _p(d["gl"]) if mode != "no_gl" else None, n, _p(gb), _p(gt), _p(gs), _p(ws), _stream())
    assert rc == 0
    return gb, gt, gs


# ---- kernels against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gn_forward(shape, regime):
    d, runs = gn_case(shape, regime)
    (ref, _), (chain, _) = runs["both"]
    got = native_gn_fwd(d)
    for name, k, c, r in zip(("out", "loss", "mean", "rstd"), got, chain, ref):
        within_bar("%s %s" % (regime, name), k, c, r)


@pytest.mark.parametrize("mode", ["both", "no_go", "no_gl", "no_twin"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gn_backward(shape, regime, mode):
    d, runs = gn_case(shape, regime)
    (_, ref), (_, chain) = runs[mode]
    got = native_gn_bwd(d, native_gn_fwd(d), mode)
    for name, k, c, r in zip(("g_branch", "g_twin", "g_scaling", "g_gamma", "g_beta"), got, chain, ref):
        if k is None:
            assert name == "g_twin" and mode == "no_twin"
            continue
        within_bar("%s %s %s" % (regime, mode, name), k, c, r)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_forward(n, regime):
    d, runs = l1_case(n, regime)
    (ref, _), (chain, _) = runs["both"]
    for name, k, c, r in zip(("out", "loss"), native_l1_fwd(d), chain, ref):
        within_bar("%s %s" % (regime, name), k, c, r)


@pytest.mark.parametrize("mode", ["both", "no_go", "no_gl"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_backward(n, regime, mode):
    d, runs = l1_case(n, regime)
    (_, ref), (_, chain) = runs[mode]
    for name, k, c, r in zip(("g_branch", "g_twin", "g_scaling"), native_l1_bwd(d, mode), chain, ref):
        within_bar("%s %s %s" % (regime, mode, name), k, c, r)


def test_sign_at_zero():
    """exact zeros in y_branch: sign(scaling * y_branch) = 0 there, so d/dy_branch is scaling * dx alone (with grad_out NULL the
    loss term +-grad_loss / N would otherwise be most of it); y_twin, gamma and beta stay random"""
    shape = (2, 256, 35)
    d = dict(_inputs(shape, "o1", 31, True))
    planted = torch.zeros(shape, dtype=torch.bool, device=dev())
    planted.view(-1)[::7] = True
    d["yb"] = d["yb"].masked_fill(planted, 0.0)
    leaves = [d[k] for k in ("yb", "yt", "s", "gamma", "beta")]
    for mode in ("no_go", "both"):
        _, ref = chain_run(gn_chain, [t.double() for t in leaves], d["go"], d["gl"], mode)
        _, chain = chain_run(gn_chain, leaves, d["go"], d["gl"], mode)
        got = native_gn_bwd(d, native_gn_fwd(d), mode)
        sel = planted.reshape(-1)
        within_bar("planted %s g_branch" % mode, got[0], chain[0], ref[0], sel)
        # ... and against the op chain itself at those positions, the same bar
        diff = float((got[0] - chain[0]).abs().reshape(-1)[sel].max())
        bar = 2.0 * float((chain[0].double() - ref[0]).abs().max()) + ulp(ref[0])
        print("planted %s |kernel - chain| %.3e  bar %.3e" % (mode, diff, bar))
        assert diff <= bar
    dl = dict(_inputs((12345,), "o1", 32, False))
    pl = torch.zeros(12345, dtype=torch.bool, device=dev())
    pl[::5] = True
    dl["yb"] = dl["yb"].masked_fill(pl, 0.0)
    ll = [dl[k] for k in ("yb", "yt", "s")]
    _, ref = chain_run(l1_chain, [t.double() for t in ll], dl["go"], dl["gl"], "no_go")
    _, chain = chain_run(l1_chain, ll, dl["go"], dl["gl"], "no_go")
    within_bar("planted l1 g_branch", native_l1_bwd(dl, "no_go")[0], chain[0], ref[0], pl)


@pytest.mark.parametrize("shape", [(2, 256, 221), (1, 256, 16700)], ids=lambda s: "x".join(map(str, s)))
def test_determinism(shape):
    d, _ = gn_case(shape, "zira")
    runs = []
    for _ in range(2):
        fwd = native_gn_fwd(d)
        runs.append(list(fwd) + list(native_gn_bwd(d, fwd, "both")))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    dl, _ = l1_case(L1_SIZES[-1], "zira")
    runs = [list(native_l1_fwd(dl)) + list(native_l1_bwd(dl, "both")) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_declined_shapes():
    lib = _lib.load()
    assert lib.zira_rsb_gn_workspace_floats(2, 48, 35, 32) == 0          # C % G != 0
    assert lib.zira_rsb_gn_workspace_floats(0, 32, 35, 32) == 0
    assert lib.zira_rsb_l1_workspace_floats(0) == 0
    d = _inputs((2, 48, 35), "o1", 5, True)
    o = torch.empty_like(d["yb"])
    one, st = torch.empty(1, device=dev()), torch.empty(64, device=dev())
    assert lib.zira_rsb_gn_fwd_f32(_p(d["yb"]), _p(d["yt"]), _p(d["s"]), _p(d["gamma"]), _p(d["beta"]), 2, 48, 35, 32, EPS, _p(o),
                                   _p(one), _p(st), _p(st), _p(st), _stream()) == -1


# ---- module level ------------------------------------------------------------------------------------------------------------------
def test_modules_against_the_reference_fixtures(monkeypatch):
    """RepZeroConv2dGN (1x1; 3x3 stride 2) and RepZeroLinear with the switch on, against the reference's own classes
    (tests/golden/mod_ml_*.pt) at the tolerance the switch-off tests use; the native Functions must be what ran."""
    from test_modules_golden import _check_branch_module, load, to

    monkeypatch.setattr(ml, "NATIVE_EPILOGUE", True)
    ran = []
    for cls in (ml._GNEpilogue, ml._L1Epilogue):
        monkeypatch.setattr(cls, "apply", lambda *a, _f=cls.apply, _n=cls.__name__: (ran.append(_n), _f(*a))[1])
    _check_branch_module(ml.RepZeroLinear(24, 16), to(load("ml_rep_zero_linear"), "cuda"), "cuda")
    assert ran == ["_L1Epilogue"]
    for name in ("1x1", "3x3s2"):
        g = to(load("ml_rep_zero_conv_gn_" + name), "cuda")
        _check_branch_module(ml.RepZeroConv2dGN(12, 32, **g["kwargs"]), g, "cuda")
    assert ran == ["_L1Epilogue", "_GNEpilogue", "_GNEpilogue"]


@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_rep_round_trip_and_switch_off(monkeypatch, kind):
    torch.manual_seed(3)
    if kind == "conv":
        make = lambda: ml.RepZeroConv2dGN(12, 64, 3, stride=2, padding=1)
        x = torch.randn(2, 12, 9, 11, device=dev())
    else:
        make = lambda: ml.RepZeroLinear(24, 16)
        x = torch.randn(2, 7, 24, device=dev())
    a = make().to(dev())
    with torch.no_grad():
        for p in a.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    b = make().to(dev())
    b.load_state_dict(a.state_dict())
    # switch off (the default): exactly today's expressions, evaluated here
    assert ml.NATIVE_EPILOGUE is False
    a.train()
    out, zl = a(x)
    if kind == "conv":
        branch = F.conv2d(x, a.weight, a.bias, a.stride, a.padding) * a.scaling
        want = a.freeze_gn(branch + a.freeze_conv(x))
    else:
        branch = a.scaling * F.linear(x, a.weight, a.bias)
        want = branch + a.freeze_linear(x)
    assert torch.equal(out, want) and torch.equal(zl, branch.abs().mean() + want.abs().mean())
    assert "Epilogue" not in type(out.grad_fn).__name__
    # __rep__ after the same state: the merge does not depend on the switch
    monkeypatch.setattr(ml, "NATIVE_EPILOGUE", True)
    b.train()
    out_on, _ = b(x)
    assert "Epilogue" in type(out_on.grad_fn).__name__
    a.__rep__()
    b.__rep__()
    assert list(a.state_dict()) == list(b.state_dict())
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(va, vb), k


def test_eval_and_other_dtypes_keep_the_op_chain(monkeypatch):
    monkeypatch.setattr(ml, "NATIVE_EPILOGUE", True)
    conv = ml.RepZeroConv2dGN(12, 32, 1).to(dev())
    x = torch.randn(2, 12, 5, 7, device=dev())
    conv.eval()
    out, zl = conv(x)
    assert torch.equal(out, conv.freeze_conv(x)) and float(zl) == 0.0
    conv.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, _ = conv(x)
    assert "Epilogue" not in type(out.grad_fn).__name__
    out, _ = conv.double()(x.double())
    assert out.dtype == torch.float64 and "Epilogue" not in type(out.grad_fn).__name__
