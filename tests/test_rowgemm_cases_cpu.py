"""The cases of the row GEMM's GPU test (tests/rowgemm_cases.py), proven where there is no GPU: the float64 references agree
with float64 autograd of the nn.Linear / F.layer_norm / ReLU compositions they stand for, the dispatch mirror over the cases
reaches every instantiation of the launcher, and every rowgemm() call of the model has a case of its form and flags."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import rowgemm_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [rc.case_id(c) for c in rc.CASES]


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _qb(c, x):
    """[m, C] in logical order as [Q, B, C], the way the decoder holds it."""
    B = c.batch if c.batch else 1
    return x.reshape(c.m // B, B, x.shape[-1])


def _forward_composition(c, t):
    """The forward calls, composed from F.linear / relu / F.layer_norm in float64.  Batch-first operands go through
    transpose(0, 1) of [Q, B, C] tensors, not through the index map of the references."""
    a = t.a_mem.double()
    if "a_batch_first" in c.flags:
        Q = c.m // c.batch
        a = a.reshape(c.batch, Q, c.k).transpose(0, 1).reshape(c.m, c.k)
    w_nk = (t.w if c.nk else t.w.t()).double()                                   # nn.Linear(k, n).weight
    bias = None if t.bias is None else t.bias.double()
    if t.pos is not None:
        pc = rc.pos_cols(c)
        y = torch.cat([F.linear(a + t.pos.double(), w_nk[:pc], None if bias is None else bias[:pc]),
                       F.linear(a, w_nk[pc:], None if bias is None else bias[pc:])], -1)
    else:
        y = F.linear(a, w_nk, bias)
    if t.res is not None:
        y = y + t.res.double()
    pre = y
    if "relu" in c.flags:
        y = F.relu(y)
    ln = None
    if "ln" in c.flags:
        ln = F.layer_norm(y, (c.n,), t.ln_gamma.double(), t.ln_beta.double(), rc.LN_EPS)
    if "c_batch_first" in c.flags:
        y = _qb(c, y).transpose(0, 1).reshape(c.m, c.n)
    return pre, y, ln


def _backward_composition(c, t):
    """The gradient calls (mask and / or lnb) from autograd in float64: c is the gradient of u in

        s = r0 + F.linear(relu(u), Wop)      y = F.layer_norm(s) * gamma      (lnb)      or      y = s      (mask alone)

    for the upstream gradient a, with Wop = op(W) [K, N] the weight of nn.Linear(N, K); lnb_dx is the gradient of r0."""
    Wop = rc.op_w(c, t.w).double()
    if t.mask is not None:
        u = t.mask.double().clone().requires_grad_()
        hidden = F.relu(u)
    else:
        u = torch.randn(c.m, c.n, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).requires_grad_()
        hidden = u
    lin = F.linear(hidden, Wop)
    if "lnb" in c.flags:
        r0 = (t.lnb_x.double() - lin.detach()).requires_grad_()                   # so that s is x, to rounding
        y = F.layer_norm(r0 + lin, (c.k,), t.lnb_gamma.double(), None, rc.LN_EPS)
        gu, gr0 = torch.autograd.grad(y, [u, r0], t.a.double())
    else:
        (gu,), gr0 = torch.autograd.grad(lin, [u], t.a.double()), None
    if "c_batch_first" in c.flags:
        gu = _qb(c, gu).transpose(0, 1).reshape(c.m, c.n)
    return gu, gr0


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_references_agree_with_float64_autograd(c):
    t = rc.inputs(c)
    if "lnb" in c.flags or "mask" in c.flags:
        assert t.pos is None and t.bias is None and t.res is None and "relu" not in c.flags
        want_c, want_dx = _backward_composition(c, t)
        if "lnb" in c.flags:
            xd = t.lnb_x.double()
            mean, rstd = xd.mean(-1), (xd.var(-1, unbiased=False) + rc.LN_EPS).rsqrt()     # the statistics autograd uses
            dx = rc.layernorm_bwd_f64(t.a, t.lnb_x, t.lnb_gamma, mean, rstd)
            assert _rel(dx, want_dx) < 1e-12
            # the float32 statistics the kernel is handed are those, rounded once
            assert float(((t.lnb_mean.double() - mean).abs() / (mean.abs() + 1)).max()) < rc.U
            assert float(((t.lnb_rstd.double() - rstd).abs() / rstd).max()) < rc.U
            W = rc.op_w(c, t.w).double()
            pre = dx @ W
        else:
            pre, _ = rc.product_f64(c, t)
        got = rc.to_memory(c, rc.activate(c, t, pre))
        assert _rel(got, want_c) < 1e-12
        if t.mask is not None:     # the planted entries are zeroed, and would not have been
            flat = rc.activate(c, t, pre).reshape(-1)
            assert float(flat[t.planted].abs().max()) == 0.0 and float(pre.reshape(-1)[t.planted].abs().min()) > 0.0
            assert bool((t.mask.reshape(-1)[t.planted] <= 0).all())
        return
    pre, bound = rc.product_f64(c, t)
    want_pre, want_y, want_ln = _forward_composition(c, t)
    assert _rel(pre, want_pre) < 1e-12
    out = rc.activate(c, t, pre)
    if "ln" in c.flags:
        y, mean, rstd = rc.layernorm_f64(out, t.ln_gamma, t.ln_beta)
        assert _rel(y, want_ln) < 1e-12
        assert _rel(mean, want_y.mean(-1)) < 1e-12
        assert _rel(rstd, (want_y.var(-1, unbiased=False) + rc.LN_EPS).rsqrt()) < 1e-12
    else:
        assert _rel(rc.to_memory(c, out), want_y) < 1e-12


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_bound_holds_for_float32_products_in_any_order(c):
    """The bound is derived, not fitted: the same product in float32, summed forwards and backwards and in blocks of 16,
    stays inside it (the GPU test asks the same of the kernel)."""
    t = rc.inputs(c)
    if "lnb" in c.flags:
        operand = rc.layernorm_bwd_f64(t.a, t.lnb_x, t.lnb_gamma, t.lnb_mean, t.lnb_rstd).float()
        pre, bound = rc.product_f64(c, t, operand=operand)
        a32 = [operand] * 2
    else:
        pre, bound = rc.product_f64(c, t)
        a32 = [t.a + t.pos, t.a] if t.pos is not None else [t.a] * 2
    W = rc.op_w(c, t.w)
    pc = rc.pos_cols(c) if t.pos is not None else c.n
    assert float(bound.min()) > 0.0
    for order in ("forward", "backward", "chunks"):
        idx = torch.arange(c.k) if order != "backward" else torch.arange(c.k - 1, -1, -1)
        parts = []
        for a, cols in ((a32[0], slice(0, pc)), (a32[1], slice(pc, c.n))):
            if order == "chunks":
                acc = torch.zeros(c.m, W[:, cols].shape[1])
                for k0 in range(0, c.k, 16):
                    acc = acc + a[:, k0:k0 + 16] @ W[k0:k0 + 16, cols]
                parts.append(acc)
            else:
                parts.append(a[:, idx] @ W[idx][:, cols])
        got = torch.cat(parts, -1)
        if t.bias is not None:
            got = got + t.bias
        if t.res is not None:
            got = got + t.res
        ratio = float(((got.double() - pre).abs() / bound).max())
        assert ratio <= 1.0, (order, ratio)


def test_cases_cover_every_instantiation_of_the_launcher():
    reached = {c.form[:5] for c in rc.CASES}
    assert reached == rc.INSTANTIATIONS and len(reached) == 9
    src = open(os.path.join(ROOT, "ziragroundingdino_amd", "csrc", "rowgemm.hip")).read()
    named = set()
    for nk, bm, tw, lnb, depth in re.findall(r"launch\(rowgemm_kernel<(true|false), (\d+), (\d+), (true|false), (\d+)>\)", src):
        named.add((nk == "true", int(bm), int(tw), lnb == "true", int(depth)))
    assert named == rc.INSTANTIATIONS                                            # the mirror's list is the launcher's
    # threads and columns per block follow the form: 8 waves x 32 columns with the LayerNorm epilogue, else 4 waves x 16 TW
    for c in rc.CASES:
        nk, bm, tw, lnb, depth, threads, cols = c.form
        assert cols == (256 if "ln" in c.flags else 64 * tw) and threads == (512 if "ln" in c.flags else 256)
        assert c.n % cols == 0 and c.k % 128 == 0 and c.k <= 2048
        assert (c.k // 16) % depth == 0                                          # whole rounds of the ring
        assert (bm * (c.k + 4) + 256) * 4 <= 160 * 1024                          # the block's LDS
    by_name = {c.name: c for c in rc.CASES}
    assert by_name["nk32-k1024"].form[1] == 32 and (32 * 1028 + 256) * 4 == 132608 > 64 * 1024


def test_mirror_brackets_the_narrow_switch():
    lo, hi = (next(c for c in rc.CASES if c.name == n) for n in rc.SWITCH_PAIR)
    assert (lo.m, hi.m) == (5088, 5089) and lo.n == hi.n == 128 and lo.flags == hi.flags
    assert lo.form[:5] == (False, 32, 1, False, 8) and lo.form[6] == 64
    assert hi.form[:5] == (False, 32, 2, False, 8) and hi.form[6] == 128
    assert (lo.m + 31) // 32 * (lo.n // 128) == 159 and (hi.m + 31) // 32 * (hi.n // 128) == 160


def test_every_case_has_a_ragged_last_row_block():
    for c in rc.CASES:
        if c.name == rc.SWITCH_PAIR[0]:
            assert c.m % c.form[1] == 0       # 159 whole blocks: what the switch fixes
            continue
        assert c.m % c.form[1] != 0, c.name
        assert c.m > c.form[1], c.name                                           # more than one row block
        if c.batch:
            assert c.m % c.batch == 0 and c.batch > 1
        assert bool(c.batch) == bool(c.flags & {"a_batch_first", "c_batch_first"})


def test_every_call_of_the_model_has_a_case_of_its_form_and_flags():
    # the table is the source's: every line it names holds a call, and there is no call it does not name
    pkg = os.path.join(ROOT, "ziragroundingdino_amd")
    for fname in ("decoder_layer.py", "dense.py"):
        lines = open(os.path.join(pkg, fname)).read().split("\n")
        calls = {i + 1 for i, line in enumerate(lines) if re.search(r"(?<![\w.])rowgemm\(", line) and not line.lstrip().startswith("def ")}
        listed = {int(d.where.split(":")[1]) for d in rc.DECODER_CALLS if d.where.startswith(fname + ":")}
        assert calls == listed, (fname, sorted(calls ^ listed))
        for ln_no in listed:
            assert "w_is_nk=False" in lines[ln_no - 1]
    for d in rc.DECODER_CALLS:
        for m in rc.ROW_COUNTS[d.rows]:
            f = rc.form(m, d.n, d.k, False, "ln" in d.flags, "lnb" in d.flags)
            hits = [c.name for c in rc.CASES if c.form == f and c.flags == d.flags]
            assert hits, (d.where, m, f, sorted(d.flags))
            if "pos" in d.flags:      # the model's pos_cols end on a block boundary of the launch
                assert (d.pos_cols or d.n) % f[6] == 0 or (d.pos_cols or d.n) >= d.n


def test_pos_cols_lies_on_a_block_boundary():
    n_pos = 0
    for c in rc.CASES:
        if "pos" not in c.flags:
            assert c.pos_cols is None
            continue
        n_pos += 1
        pc = rc.pos_cols(c)
        assert 0 < pc <= c.n and pc % c.form[6] == 0, c.name
        assert ("pos_partial" in c.flags) == (pc < c.n)
    assert n_pos >= 6
    c = next(c for c in rc.CASES if c.name == "kn32n-deep-pos128")
    assert c.n // c.form[6] == 4 and rc.pos_cols(c) // c.form[6] == 2             # blocks 0 and 1 of four take the code


def test_relu_kink_band_stays_under_its_cap():
    """Entries of the ReLU cases whose pre-activation lies within its own bound of zero, where the kernel may land on either
    side: at most 0.1 % of a case's entries.  Counts: kn32n-deep-k512-relu 5 of 12800."""
    seen = {}
    for c in rc.CASES:
        if "relu" not in c.flags:
            continue
        t = rc.inputs(c)
        pre, bound = rc.product_f64(c, t)
        band = rc.kink_band(c, t, pre, bound)
        seen[c.name] = band
        assert band <= 1e-3 * c.m * c.n, (c.name, band)
        assert int(rc.exact_zero(c, t, pre, bound).sum()) > 0.4 * c.m * c.n      # and the ReLU does cut
    assert seen == {"kn32n-deep-k512-relu": 5}, seen


def test_masks_hold_signed_zeros_and_a_negative_value():
    for c in rc.CASES:
        if "mask" not in c.flags:
            continue
        t = rc.inputs(c)
        v = t.mask.reshape(-1)[t.planted]
        neg_zero = (v == 0) & torch.signbit(v)
        pos_zero = (v == 0) & ~torch.signbit(v)
        assert int(neg_zero.sum()) >= 8 and int(pos_zero.sum()) >= 8 and int((v < 0).sum()) >= 8, c.name
        assert float(t.mask.reshape(-1)[-1]) == 0.0 and bool(torch.signbit(t.mask.reshape(-1)[-1]))


def test_row_map_is_the_headers():
    perm = rc.mem_rows(6, 3)          # Q = 2, B = 3: logical r = q * 3 + b lives at b * 2 + q
    assert perm.tolist() == [0, 2, 4, 1, 3, 5]
    for c in rc.CASES:
        if "a_batch_first" in c.flags:
            t = rc.inputs(c)
            Q = c.m // c.batch
            for q, b in ((0, 0), (Q - 1, c.batch - 1), (3, 1)):
                assert torch.equal(t.a_mem[b * Q + q], t.a[q * c.batch + b])
