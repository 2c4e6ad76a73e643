"""zira_rowgemm_f32 (csrc/rowgemm.hip) through its C ABI in every form the launcher can choose, those the decoder runs
(w_is_nk = 0) first: tests/rowgemm_cases.py holds the cases, the float64 references and the derived error bounds, proven on
the CPU by test_rowgemm_cases_cpu.py.

Each piece is held to its own reference: the product to an elementwise bound that any float32 summation order satisfies, the
LayerNorm epilogue to a float64 LayerNorm of the kernel's own pre-normalisation rows, the LayerNorm-backward prologue to the
float64 formula on the same float32 operands and the product behind it to float64 of the returned dx.  No share of wrong rows
is allowed.  Every output is a slice of a larger buffer filled with a sentinel; every case runs twice, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import rowgemm_cases as rc  # noqa: E402
from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd.rowgemm import rowgemm  # noqa: E402

SENTINEL = 12345.5
PAD_ROWS = 40        # rows behind the m the kernel is told of (more than a block of 32)
GUARD_COLS = 8       # columns behind the n of a row-strided c
LN_TOL = 2e-5        # test_layernorm_gpu.py: float32 rounding of a two-pass LayerNorm at this input scale
LNB_TOL = 2e-6       # test_layernorm_gpu.py::test_input_gradient_kernel_matches_float64, of the largest entry
IDS = [rc.case_id(c) for c in rc.CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _to(t, dev):
    d = type(t)()
    for k, v in vars(t).items():
        setattr(d, k, v.to(dev) if isinstance(v, torch.Tensor) else v)
    return d


def _buffers(c, dev, save):
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev, dtype=torch.float32)
    b = {"c": full(c.m + PAD_ROWS, c.n + GUARD_COLS)}
    if save and "ln" in c.flags:
        b.update(ln_sum=full(c.m + PAD_ROWS, c.n), ln_mean=full(c.m + PAD_ROWS), ln_rstd=full(c.m + PAD_ROWS))
    if save and "lnb" in c.flags:
        b.update(lnb_dx=full(c.m + PAD_ROWS, c.k))
    return b


def _args(c, d, b, pos_cols=None):
    """zira_rowgemm_args filled field by field, the way rowgemm() fills them, with the outputs pointing into `b`."""
    f = c.flags
    a = _lib.RowGemmArgs()
    a.a, a.lda = d.a_mem.data_ptr(), c.k
    if d.pos is not None:
        a.pos, a.ldpos, a.pos_cols = d.pos.data_ptr(), c.k, rc.pos_cols(c) if pos_cols is None else pos_cols
    a.w, a.ldw, a.w_is_nk = d.w.data_ptr(), d.w.stride(0), int(c.nk)
    if d.bias is not None:
        a.bias = d.bias.data_ptr()
    if d.res is not None:
        a.res, a.ldres = d.res.data_ptr(), c.n
    if d.mask is not None:
        a.mask = d.mask.data_ptr()
    a.relu = int("relu" in f)
    if "ln" in f:
        a.ln_gamma, a.ln_beta, a.ln_eps = d.ln_gamma.data_ptr(), d.ln_beta.data_ptr(), rc.LN_EPS
        if "ln_sum" in b:
            a.ln_sum, a.ln_mean, a.ln_rstd = b["ln_sum"].data_ptr(), b["ln_mean"].data_ptr(), b["ln_rstd"].data_ptr()
    if "lnb" in f:
        a.lnb_x, a.lnb_gamma = d.lnb_x.data_ptr(), d.lnb_gamma.data_ptr()
        a.lnb_mean, a.lnb_rstd = d.lnb_mean.data_ptr(), d.lnb_rstd.data_ptr()
        if "lnb_dx" in b:
            a.lnb_dx = b["lnb_dx"].data_ptr()
    a.c, a.ldc = b["c"].data_ptr(), b["c"].stride(0)
    a.m, a.n, a.k = c.m, c.n, c.k
    a.batch, a.a_batch_first, a.c_batch_first = c.batch, int("a_batch_first" in f), int("c_batch_first" in f)
    return a


def _launch(c, d, dev, save=True):
    b = _buffers(c, dev, save)
    rcode = _lib.load().zira_rowgemm_f32(_args(c, d, b), torch.cuda.current_stream(dev).cuda_stream)
    assert rcode == 0, rcode
    return b


def _wrapper(c, d, dev, save):
    """The same call through rowgemm(), c into a slice of a sentinel-filled buffer with out=."""
    f = c.flags
    buf = torch.full((c.m + PAD_ROWS, c.n + GUARD_COLS), SENTINEL, device=dev, dtype=torch.float32)
    ret = rowgemm(d.a_mem, d.w, w_is_nk=c.nk, bias=d.bias, pos=d.pos, pos_cols=c.pos_cols or 0, res=d.res, mask=d.mask,
                  relu="relu" in f, ln=(d.ln_gamma, d.ln_beta, rc.LN_EPS) if "ln" in f else None, ln_save=save and "ln" in f,
                  lnb=(d.lnb_x, d.lnb_gamma, d.lnb_mean, d.lnb_rstd) if "lnb" in f else None, lnb_save=save and "lnb" in f,
                  batch=c.batch, a_batch_first="a_batch_first" in f, c_batch_first="c_batch_first" in f, out=buf[:c.m, :c.n])
    return buf, ret


def _untouched(c, b):
    """Rows beyond m of every output and the guard columns of c keep the sentinel."""
    assert bool((b["c"][c.m:] == SENTINEL).all()), "c: rows beyond m were written"
    assert bool((b["c"][:, c.n:] == SENTINEL).all()), "c: guard columns were written"
    for name in ("ln_sum", "ln_mean", "ln_rstd", "lnb_dx"):
        if name in b:
            assert bool((b[name][c.m:] == SENTINEL).all()), name + ": rows beyond m were written"


def _within(name, c, got, want, bound, zero=None):
    """|got - want| <= bound elementwise, exact zeros where asked; reports the largest share of the bound used."""
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
    ratio = (got.double() - want).abs() / bound
    worst = float(ratio.max())
    print("%s %s: largest |err| / bound = %.3g" % (c.name, name, worst))
    if worst > 1.0:
        r, col = divmod(int(ratio.argmax()), got.shape[1])
        raise AssertionError("%s: %d entries outside the bound; worst %.3g x bound at row %d column %d (got %r, want %r)" % (
            name, int((ratio > 1.0).sum()), worst, r, col, float(got[r, col]), float(want[r, col])))
    if zero is not None:
        assert float(got[zero].abs().max()) == 0.0, name + ": a masked / rectified entry is not exactly zero"


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_case_matches_float64(c):
    dev = _dev()
    t = rc.inputs(c)
    d = _to(t, dev)
    b = _launch(c, d, dev)
    b2 = _launch(c, d, dev)
    for name in b:
        assert torch.equal(b[name], b2[name]), name + ": two runs differ"
    _untouched(c, b)
    perm = rc.mem_rows(c.m, c.batch) if "c_batch_first" in c.flags else torch.arange(c.m)
    got_c = b["c"][:c.m, :c.n].cpu()[perm]                       # logical row r from memory row b * Q + q
    if "ln" in c.flags:
        pre, bound = rc.product_f64(c, t)
        s = b["ln_sum"][:c.m].cpu()
        _within("ln_sum", c, s, rc.activate(c, t, pre), bound)
        y, mean, rstd = rc.layernorm_f64(s, t.ln_gamma, t.ln_beta)      # of the kernel's own sums
        err_y = float((got_c.double() - y).abs().max())
        err_mean = float((b["ln_mean"][:c.m].cpu().double() - mean).abs().max())
        err_rstd = float(((b["ln_rstd"][:c.m].cpu().double() - rstd).abs() / rstd).max())
        print("%s layernorm: c %.3g, mean %.3g (abs), rstd %.3g (rel); tolerance %.1g" % (c.name, err_y, err_mean, err_rstd, LN_TOL))
        assert err_y < LN_TOL and err_mean < LN_TOL and err_rstd < LN_TOL
    elif "lnb" in c.flags:
        dx = b["lnb_dx"][:c.m].cpu()
        want_dx = rc.layernorm_bwd_f64(t.a, t.lnb_x, t.lnb_gamma, t.lnb_mean, t.lnb_rstd)
        err_dx = float((dx.double() - want_dx).abs().max() / want_dx.abs().max())
        print("%s lnb_dx: %.3g of the largest entry; tolerance %.1g" % (c.name, err_dx, LNB_TOL))
        assert bool(torch.isfinite(dx).all()) and err_dx < LNB_TOL
        pre, bound = rc.product_f64(c, t, operand=dx)
        _within("c", c, got_c, rc.activate(c, t, pre), bound, rc.exact_zero(c, t, pre, bound) if t.mask is not None else None)
    else:
        pre, bound = rc.product_f64(c, t)
        zero = rc.exact_zero(c, t, pre, bound)
        _within("c", c, got_c, rc.activate(c, t, pre), bound, zero if bool(zero.any()) else None)
    # through rowgemm(), with and without the saved arrays: the same bits
    for save in (True, False):
        buf, ret = _wrapper(c, d, dev, save)
        assert torch.equal(buf, b["c"]), "rowgemm(out=) with save=%s differs from the ABI call" % save
        extras = list(ret[1:]) if isinstance(ret, tuple) else []
        names = [n for n in ("ln_sum", "ln_mean", "ln_rstd", "lnb_dx") if n in b] if save else []
        assert len(extras) == len(names)
        for name, e in zip(names, extras):
            assert torch.equal(e, b[name][:c.m]), name
    # and from the ABI without them
    if c.flags & {"ln", "lnb"}:
        b3 = _launch(c, d, dev, save=False)
        assert torch.equal(b3["c"], b["c"])


def _pos_case(name):
    base = next(c for c in rc.CASES if c.name == name)
    c = rc._case(base.name, base.m, base.n, base.k, nk=base.nk, batch=base.batch, **{f: True for f in base.flags | {"pos"}})
    t = rc.inputs(base)
    t.pos = torch.randn(c.m, c.k, generator=torch.Generator().manual_seed(17))
    return c, t


@pytest.mark.parametrize("name", ["kn16-ln", "nk16-ln-k128", "kn32n-deep-bias", "nk32-k1024"])
def test_position_code_without_columns_is_refused(name):
    """pos set with pos_cols <= 0 through the ABI: -3, nothing launched (rowgemm() maps its own pos_cols=0 to N)."""
    dev = _dev()
    c, t = _pos_case(name)
    d = _to(t, dev)
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    for pc in (0, -128):
        b = _buffers(c, dev, True)
        assert lib.zira_rowgemm_f32(_args(c, d, b, pos_cols=pc), st) == -3
        torch.cuda.synchronize()
        for name_, buf in b.items():
            assert bool((buf == SENTINEL).all()), name_
    # the wrapper's pos_cols = 0 is every column, as pos_cols = N and anything beyond through the ABI
    b = _launch(c, d, dev)
    buf, _ = _wrapper(c, d, dev, True)
    assert torch.equal(buf, b["c"])
    b2 = _buffers(c, dev, True)
    assert lib.zira_rowgemm_f32(_args(c, d, b2, pos_cols=c.n + 128), st) == 0
    assert torch.equal(b2["c"], b["c"])
    pre, bound = rc.product_f64(c, t)
    if "ln" in c.flags:
        _within("ln_sum", c, b["ln_sum"][:c.m].cpu(), pre, bound)
    else:
        _within("c", c, b["c"][:c.m, :c.n].cpu(), pre, bound)


@pytest.mark.parametrize("name", ["kn16-ln", "nk16-ln-k128"])
def test_position_code_on_half_a_layernorm_block_is_refused(name):
    """With the LayerNorm epilogue one block owns all 256 columns and stages one A: pos_cols = 128 cannot be served."""
    dev = _dev()
    c, t = _pos_case(name)
    d = _to(t, dev)
    b = _buffers(c, dev, True)
    assert _lib.load().zira_rowgemm_f32(_args(c, d, b, pos_cols=128), torch.cuda.current_stream(dev).cuda_stream) == -3
    torch.cuda.synchronize()
    for name_, buf in b.items():
        assert bool((buf == SENTINEL).all()), name_
    with pytest.raises(RuntimeError):
        rowgemm(d.a_mem, d.w, w_is_nk=c.nk, bias=d.bias, pos=d.pos, pos_cols=128, res=d.res, ln=(d.ln_gamma, d.ln_beta, rc.LN_EPS))
