"""Inputs and references for the tests of the fused small attention (csrc/attn.hip), shared by the CPU test that proves
the inputs (test_attn_cases_cpu.py) and the GPU tests that run the kernels on them (test_attn_gpu.py).

Layouts as in the C ABI: q [L, B, H*32], k / v [S, B, H*32], additive key mask [B, S] (0 or -inf), lse [B, H, L]."""
import math
import types

import torch

D = 32          # head width of the kernels
CODE_BITS = 10  # code(j) tells 1024 keys apart

# (L, S, B, H, masked): `masked` = number of masked keys at the end of each image's key range, or None for no mask at all.
# Each shape is the smallest that reaches its branch of the launcher (S >= 256: four waves split the keys; a mask selects the
# MASK instantiation; few key blocks: dK / dV in shares of the query range + attn_sum_parts).
SHAPES = [
    (70, 256, 2, 2, (160, 1)),   # attn_fwd<4, true>: image 0 leaves wave 3 (tiles 3 and 7) nothing but masked keys
    (70, 256, 1, 2, None),       # S = 256, unmasked side of the switch
    (37, 255, 1, 2, None),       # attn_fwd<1, false> at its last S: eight tiles, the last one ragged
    (37, 255, 1, 2, (3,)),       # the same boundary, masked
    (900, 194, 1, 2, (40,)),     # long caption: 14 key blocks, 7 query shares, attn_sum_parts
    (301, 40, 1, 1, (9,)),       # B H L = 301 (no multiple of 4) with 2 shares
    (33, 289, 1, 1, None),       # attn_fwd<4> with 10 key tiles: waves 2, 3 own two; in attn_bwd_dkv waves 2, 3 own no query tile
    (5, 3, 2, 1, (1, 1)),        # one ragged tile of everything
]


def shape_id(shape):
    L, S, B, H, masked = shape
    return "L%d-S%d-B%d-H%d-%s" % (L, S, B, H, "nomask" if masked is None else "m" + "_".join(str(n) for n in masked))


def key_mask(S, B, masked):
    """Additive [B, S] mask with the last masked[b] keys of image b at -inf (None: no mask)."""
    if masked is None:
        return None
    if isinstance(masked, int):
        masked = (masked,) * B
    assert len(masked) == B
    km = torch.zeros(B, S)
    for b, n in enumerate(masked):
        if n:
            km[b, S - n:] = float("-inf")
    return km


def _heads(t, H):
    rows, B, E = t.shape
    return t.reshape(rows, B * H, E // H).transpose(0, 1)          # [B H, rows, d]


def _rows(t, B):
    BH, rows, d = t.shape
    return t.transpose(0, 1).reshape(rows, B, (BH // B) * d)        # [rows, B, H d]


def reference_f64(q, k, v, H, key_mask, scale, grad_out):
    """softmax(q k^T * scale + key_mask) v and its three gradients, written out in float64 (no autograd).

    A query whose keys are all masked has a zero output row, lse = -inf, and contributes nothing to any gradient (the
    kernels' documented convention; the probabilities of such a row are set to 0, no NaN is formed).
    Returns a namespace: out [L, B, E], lse [B, H, L], dq, dk, dv, and max_logit (largest |score| over unmasked keys)."""
    L, B, E = q.shape
    S = k.shape[0]
    qh, kh, vh, go = (_heads(t.detach().double(), H) for t in (q, k, v, grad_out))
    s = torch.bmm(qh, kh.transpose(1, 2)) * float(scale)                                    # [B H, L, S]
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :].expand(B, H, 1, S).reshape(B * H, 1, S)
    finite = torch.isfinite(s)
    max_logit = float(s[finite].abs().max()) if bool(finite.any()) else 0.0
    m = s.amax(-1, keepdim=True)
    live = m > float("-inf")
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))                            # (exp(-inf) = 0)
    den = e.sum(-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(e))
    lse = torch.where(live, m + torch.log(torch.where(live, den, torch.ones_like(den))), m).squeeze(-1)
    out = torch.bmm(p, vh)
    dv = torch.bmm(p.transpose(1, 2), go)
    dp = torch.bmm(go, vh.transpose(1, 2))
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq = torch.bmm(ds, kh) * float(scale)
    dk = torch.bmm(ds.transpose(1, 2), qh) * float(scale)
    return types.SimpleNamespace(out=_rows(out, B), lse=lse.reshape(B, H, L), dq=_rows(dq, B), dk=_rows(dk, B), dv=_rows(dv, B),
                                 max_logit=max_logit)


def composition(q, k, v, H, key_mask, scale):
    """The plain composition in the inputs' own precision, differentiable: what the kernels replace."""
    L, B, E = q.shape
    S = k.shape[0]
    s = torch.bmm(_heads(q, H), _heads(k, H).transpose(1, 2)) * scale
    if key_mask is not None:
        s = s + key_mask.to(s.dtype)[:, None, None, :].expand(B, H, 1, S).reshape(B * H, 1, S)
    return _rows(torch.bmm(s.softmax(-1), _heads(v, H)), B)


def _code(j):
    """[n, 32]: the first CODE_BITS entries are the bits of j as +-1, the rest 0."""
    j = torch.as_tensor(j, dtype=torch.int64)
    bits = (j[:, None] >> torch.arange(CODE_BITS)) & 1
    c = torch.zeros(j.numel(), D)
    c[:, :CODE_BITS] = (2 * bits - 1).float()
    return c


def pi(i, head, batch, live):
    """The key that query i of (batch, head) selects."""
    return (7 * i + 3 + head + batch) % live


def one_hot_case(L, S, B, H, n_masked, seed):
    """Inputs on which every result is exact in fp32 whatever the order of the sums (use with scale = 1.0).

    k[j] = code(j), q[i] = 64 code(pi(i)): the selected key scores 640 and every other key at most 512, and exp(-128) is 0
    in fp32, so every probability is exactly 0 or 1.  v and grad_out hold small integers.  The masked keys (the last
    n_masked of an image; an int or one count per image) are copies of live keys' k rows with v rows of their own: without
    the mask the selected key's probability would be 0.5.
    Returns a namespace with q, k, v, grad_out, key_mask (None when nothing is masked), scale, and the exact results out,
    lse, dq, dk, dv (fp32, CPU)."""
    assert S <= 2 ** CODE_BITS
    masked = (n_masked,) * B if isinstance(n_masked, int) else tuple(n_masked)
    assert len(masked) == B and all(0 <= n < S for n in masked)
    g = torch.Generator().manual_seed(seed)
    E = H * D
    v = torch.randint(-8, 9, (S, B, E), generator=g).float()
    go = torch.randint(-4, 5, (L, B, E), generator=g).float()
    q = torch.zeros(L, B, E)
    k = torch.zeros(S, B, E)
    out = torch.zeros(L, B, E)
    dv = torch.zeros(S, B, E)
    i = torch.arange(L)
    for b in range(B):
        live = S - masked[b]
        src = torch.cat([torch.arange(live), (5 * torch.arange(masked[b])) % live])     # key row -> the code it carries
        for h in range(H):
            cols = slice(h * D, (h + 1) * D)
            sel = pi(i, h, b, live)
            k[:, b, cols] = _code(src)
            q[:, b, cols] = 64.0 * _code(sel)
            out[:, b, cols] = v[sel, b, cols]
            dv[:, b, cols].index_add_(0, sel, go[:, b, cols])                              # (sums of small integers: exact)
        t = torch.arange(live, S)
        clash = (v[t, b] == v[src[t], b]).all(-1)                                          # a copy must differ in v from its original
        v[t[clash], b, 0] = torch.where(v[t[clash], b, 0] < 8, v[t[clash], b, 0] + 1, v[t[clash], b, 0] - 1)
    return types.SimpleNamespace(
        q=q, k=k, v=v, grad_out=go, key_mask=key_mask(S, B, masked) if any(masked) else None, scale=1.0, H=H,
        out=out, lse=torch.full((B, H, L), 640.0), dq=torch.zeros(L, B, E), dk=torch.zeros(S, B, E), dv=dv)


def randn_case(L, S, B, H, masked, seed, q_gain=1.0):
    """N(0, 1) inputs (q times q_gain: logits of standard deviation ~q_gain at scale 1 / sqrt(32)) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    E = H * D
    return types.SimpleNamespace(
        q=torch.randn(L, B, E, generator=g) * q_gain, k=torch.randn(S, B, E, generator=g), v=torch.randn(S, B, E, generator=g),
        grad_out=torch.randn(L, B, E, generator=g), key_mask=key_mask(S, B, masked), scale=1.0 / math.sqrt(D), H=H)
