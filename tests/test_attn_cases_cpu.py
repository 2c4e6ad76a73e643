"""The inputs of the fused attention's GPU tests (tests/attn_cases.py), proven where there is no GPU: the one-hot cases give
their exact results in fp32 torch on the CPU, bit for bit, and the float64 reference agrees with autograd of the plain
composition."""
import pytest
import torch

import attn_cases as ac


def _ids(shapes):
    return [ac.shape_id(s) for s in shapes]


def _fp32_composition_with_lse(c):
    """out, lse, dq, dk, dv of the plain composition in fp32 (autograd)."""
    q, k, v = (t.clone().requires_grad_() for t in (c.q, c.k, c.v))
    L, B, E = q.shape
    S, H = k.shape[0], c.H
    out = ac.composition(q, k, v, H, c.key_mask, c.scale)
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], c.grad_out)
    with torch.no_grad():
        s = torch.bmm(ac._heads(q, H), ac._heads(k, H).transpose(1, 2)) * c.scale
        if c.key_mask is not None:
            s = s + c.key_mask[:, None, None, :].expand(B, H, 1, S).reshape(B * H, 1, S)
        lse = torch.logsumexp(s, -1).reshape(B, H, L)
    return out.detach(), lse, dq, dk, dv


@pytest.mark.parametrize("shape", ac.SHAPES, ids=_ids(ac.SHAPES))
def test_one_hot_case_is_exact_in_fp32(shape):
    L, S, B, H, masked = shape
    c = ac.one_hot_case(L, S, B, H, masked if masked is not None else 0, seed=L + S)
    out, lse, dq, dk, dv = _fp32_composition_with_lse(c)
    assert torch.equal(out, c.out)
    assert torch.equal(lse, c.lse) and float(lse.min()) == 640.0 == float(lse.max())
    assert torch.equal(dv, c.dv)
    assert torch.equal(dq, c.dq) and torch.equal(dk, c.dk)          # (both zero; -0.0 == 0.0)
    # the float64 reference gives the same up to exp(-128) = 2.6e-56, which float64 still holds
    r = ac.reference_f64(c.q, c.k, c.v, H, c.key_mask, c.scale, c.grad_out)
    for name in ("out", "lse", "dq", "dk", "dv"):
        assert float((getattr(r, name) - getattr(c, name).double()).abs().max()) < 1e-45, name


@pytest.mark.parametrize("shape", [s for s in ac.SHAPES if s[4] is not None], ids=_ids([s for s in ac.SHAPES if s[4] is not None]))
def test_one_hot_case_needs_the_mask(shape):
    """A masked key is a copy of a live key with another v row: ignoring the mask halves the selected probability."""
    L, S, B, H, masked = shape
    c = ac.one_hot_case(L, S, B, H, masked, seed=L + S)
    for b, n in enumerate(masked):
        live = S - n
        for t in range(n):
            assert torch.equal(c.k[live + t, b], c.k[(5 * t) % live, b])
            assert not torch.equal(c.v[live + t, b], c.v[(5 * t) % live, b])
    r = ac.reference_f64(c.q, c.k, c.v, H, None, c.scale, c.grad_out)
    assert not torch.equal(r.out, c.out.double())
    assert float(r.lse.max()) > 640.0


@pytest.mark.parametrize("shape", ac.SHAPES, ids=_ids(ac.SHAPES))
@pytest.mark.parametrize("q_gain", [1.0, 16.0])
def test_reference_f64_agrees_with_autograd(shape, q_gain):
    L, S, B, H, masked = shape
    c = ac.randn_case(L, S, B, H, masked, seed=3 * L + S, q_gain=q_gain)
    r = ac.reference_f64(c.q, c.k, c.v, H, c.key_mask, c.scale, c.grad_out)
    q, k, v = (t.double().requires_grad_() for t in (c.q, c.k, c.v))
    out = ac.composition(q, k, v, H, c.key_mask, c.scale)
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], c.grad_out.double())
    for name, got, want in (("out", r.out, out.detach()), ("dq", r.dq, dq), ("dk", r.dk, dk), ("dv", r.dv, dv)):
        err = float((got - want).abs().max() / want.abs().max())
        assert err < 1e-12, (name, err)
    s = torch.einsum("lbhd,sbhd->bhls", q.detach().reshape(L, B, H, 32), k.detach().reshape(S, B, H, 32)) * c.scale
    if c.key_mask is not None:
        s = s + c.key_mask.double()[:, None, None, :]
    assert float((r.lse - torch.logsumexp(s, -1)).abs().max()) < 1e-12
    assert r.max_logit == pytest.approx(float(s[torch.isfinite(s)].abs().max()), rel=1e-12)


def test_reference_f64_fully_masked_image_contributes_nothing():
    """Image 0 has every key masked: zero output rows, lse = -inf, zero gradients, no NaN; image 1 is what it is alone."""
    L, S, B, H = 9, 8, 2, 2
    c = ac.randn_case(L, S, B, H, (S, 3), seed=11)
    r = ac.reference_f64(c.q, c.k, c.v, H, c.key_mask, c.scale, c.grad_out)
    for t in (r.out, r.dq, r.dk, r.dv):
        assert bool(torch.isfinite(t).all())
        assert float(t[:, 0].abs().max()) == 0.0
    assert bool((r.lse[0] == float("-inf")).all()) and bool(torch.isfinite(r.lse[1]).all())
    one = ac.reference_f64(c.q[:, 1:], c.k[:, 1:], c.v[:, 1:], H, c.key_mask[1:], c.scale, c.grad_out[:, 1:])
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(getattr(r, name)[:, 1:], getattr(one, name)), name
