"""Inputs and references for the tests of the fused text side (csrc/textside.hip), shared by the CPU test that proves them
(test_textside_cases_cpu.py) and the GPU tests that run the four entry points on them (test_textside_gpu.py).

Layouts as in the C ABI (include/zira_msda.h): l_in, l_ln, out and their gradients [B, T, Dl]; a [B, Dv, H T]; c and colsum
[B, H T]; z and u [B, H T, Dv]; stats [B T, 2] = (mean, rstd); W1 [Dl, N1] = [A | C | Z] with N1 = 2 H Dv + H; O [H Dv, Dl];
keep [B] or None.  M = B T rows, HD = H Dv."""
import types

import torch
import torch.nn.functional as F

TR, TC, KC = 32, 32, 128    # the kernels' tile: rows, columns, K per chunk
MAX_DL = 256
EPS = 1e-5

# (B, T, H, Dv, Dl, note): each the smallest shape that reaches what its note names (test_textside_cases_cpu.py holds the notes'
# figures to geometry()).
SHAPES = [
    (2, 32, 4, 256, 256, "model widths | 17 K parts: 8 a chunks, the mixed chunk at 1024 holds c and z only, Z chunks, the last "
                         "with kn = 4; two forward K chunks"),
    (1, 195, 4, 256, 256, "longest caption | M = 195 = 6 x 32 + 3: seven row tiles, the last of 3 rows"),
    (3, 9, 3, 32, 96, "mixed chunk with a | HD = 96, N1 = 195: chunk 0 holds a 0..95, c 96..98, z 99..127; chunk 1 is Z with "
                      "kn = 67; Dl <= 128: one forward chunk; M = 27: one partial row tile over three images"),
    (2, 5, 3, 85, 100, "two mixed chunks | HD = 255, N1 = 513: chunk 0 a, chunk 1 mixed (a 128..254, c 255), chunk 2 mixed again "
                       "(c 256..257, z from 258): c straddles a chunk boundary; last chunk kn = 1; Dl = 100: the column tile hangs "
                       "over by 28, LayerNorm lanes beyond Dl; Dv = 85 is odd"),
    (2, 33, 2, 40, 200, "short second chunk | M = 66: the last row tile has 2 rows; Dl = 200: second forward chunk of 72; HD = 80: "
                        "one out-forward part with kn = 80; Dv < 64 in the colsum backward"),
    (5, 13, 8, 20, 256, "row tile over three images | M = 65; HD = 160: chunk 0 a, chunk 1 mixed (a 128..159, c 160..167, z "
                        "168..255), chunk 2 Z with kn = 72; keep differs per row of a tile"),
    (2, 16, 2, 64, 128, "Dl = KC | no second forward chunk; HD = 128: chunk 0 exactly an a chunk, chunk 1 mixed without a, "
                        "chunk 2 with kn = 2"),
    (2, 16, 2, 64, 129, "second chunk of one column | Dl = 129 is not a multiple of 4"),
    (1, 1, 1, 1, 4, "degenerate | one row, N1 = 3"),
]

OUTPUTS = ("l_ln", "a", "c", "z", "stats", "g_l_in", "out", "g_u", "g_colsum")
NULLABLE = ("g_a", "g_c", "g_z", "g_l_ln")


def shape_id(shape):
    B, T, H, Dv, Dl, note = shape
    return "B%d-T%d-H%d-Dv%d-Dl%d-%s" % (B, T, H, Dv, Dl, note.split(" | ")[0].replace(" ", "_"))


def _cdiv(a, b):
    return -(-a // b)


def geometry(B, T, H, Dv, Dl):
    """The launchers' arithmetic for a shape, restated from csrc/textside.hip (the four entry points and bad_dims).  None when
    the dimensions are refused.

    prep_chunks: one entry per K part of zira_text_prep_bwd_f32, (k0, kn, kind, has_a, has_c, has_z) with kind "a" (all of
    the chunk's 128 columns in a), "z" (all of it in z) or "mixed"; out_kn: the K extent of each part of
    zira_text_out_fwd_f32; fwd_chunks: the K chunks (of Dl) inside a block of the prep forward and the out backward."""
    if min(B, T, H, Dv, Dl) <= 0 or Dl > MAX_DL or B * T > 1 << 20 or H * Dv > 1 << 20:
        return None
    M, HD = B * T, H * Dv
    N1 = 2 * HD + H
    chunks = []
    for p in range(_cdiv(N1, KC)):
        k0 = p * KC
        kn = min(KC, N1 - k0)
        kind = "a" if k0 + KC <= HD else "z" if k0 >= HD + H else "mixed"
        chunks.append((k0, kn, kind, k0 < HD, k0 < HD + H and k0 + kn > HD, k0 + kn > HD + H))
    tiles = [(m0, min(TR, M - m0)) for m0 in range(0, M, TR)]
    return types.SimpleNamespace(
        M=M, HD=HD, N1=N1, prep_chunks=chunks, prep_parts=len(chunks), scratch_floats=len(chunks) * M * Dl,
        out_parts=_cdiv(HD, KC), out_kn=[min(KC, HD - k0) for k0 in range(0, HD, KC)],
        fwd_chunks=[min(KC, Dl - k0) for k0 in range(0, Dl, KC)],
        row_tiles=tiles, images_per_tile=[(m0 + n - 1) // T - m0 // T + 1 for m0, n in tiles],
        prep_col_tiles=_cdiv(N1, TC), dl_col_tiles=_cdiv(Dl, TC), dl_overhang=_cdiv(Dl, TC) * TC - Dl,
        hd_col_tiles=_cdiv(HD, TC), head_split_in_tile=any((n0 // Dv) != (min(n0 + TC, HD) - 1) // Dv for n0 in range(0, HD, TC)))


# ---- layout maps (written as index arithmetic, not as permutes: the CPU test holds them to permute / view) ------------------------

def _rows(B, T, device=None):
    m = torch.arange(B * T, device=device)
    return m // T, m % T


def scatter_acz(P, B, T, H, Dv):
    """The dense product P [M, N1] = [A | C | Z] in the kernel's layouts: a[b, d, h T + t] = A[b T + t, h Dv + d],
    c[b, h T + t] = C[b T + t, h], z[b, h T + t, d] = Z[b T + t, h Dv + d]."""
    HD = H * Dv
    b, t = _rows(B, T, P.device)
    a, c, z = P.new_zeros(B, Dv, H * T), P.new_zeros(B, H * T), P.new_zeros(B, H * T, Dv)
    for h in range(H):
        a[b, :, h * T + t] = P[:, h * Dv:(h + 1) * Dv]          # (indexed dimensions first: [M, Dv])
        c[b, h * T + t] = P[:, HD + h]
        z[b, h * T + t, :] = P[:, HD + H + h * Dv:HD + H + (h + 1) * Dv]
    return a, c, z


def gather_acz(a, c, z, B, T, H, Dv, like):
    """The inverse: [M, N1] from tensors in the layouts of a, c, z (None = zeros)."""
    HD = H * Dv
    b, t = _rows(B, T, like.device)
    G = like.new_zeros(B * T, 2 * HD + H)
    for h in range(H):
        if a is not None:
            G[:, h * Dv:(h + 1) * Dv] = a[b, :, h * T + t]
        if c is not None:
            G[:, HD + h] = c[b, h * T + t]
        if z is not None:
            G[:, HD + H + h * Dv:HD + H + (h + 1) * Dv] = z[b, h * T + t, :]
    return G


def rows_of_u(x, B, T, H, Dv):
    """[M, HD] from the layout of u [B, H T, Dv]: X[b T + t, h Dv + d] = x[b, h T + t, d]."""
    b, t = _rows(B, T, x.device)
    X = x.new_zeros(B * T, H * Dv)
    for h in range(H):
        X[:, h * Dv:(h + 1) * Dv] = x[b, h * T + t, :]
    return X


def u_of_rows(X, B, T, H, Dv):
    b, t = _rows(B, T, X.device)
    x = X.new_zeros(B, H * T, Dv)
    for h in range(H):
        x[b, h * T + t, :] = X[:, h * Dv:(h + 1) * Dv]
    return x


# ---- float64 reference, closed forms (no autograd) -----------------------------------------------------------------------------

def _keep_rows(keep, B, T, like):
    return like.new_ones(B * T, 1) if keep is None else keep.to(like).repeat_interleave(T)[:, None]


def reference_f64(case, device=None):
    """The four entry points in float64 from the formulas of include/zira_msda.h.  Returns the nine OUTPUTS."""
    d = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float64)
    B, T, H, Dv, Dl = case.B, case.T, case.H, case.Dv, case.Dl
    M = B * T
    x, lw, lb = d(case.l_in).view(M, Dl), d(case.ln_w), d(case.ln_b)
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + case.eps)
    xh = (x - mean) * rstd
    l_ln = xh * lw + lb
    a, c, z = scatter_acz(l_ln @ d(case.W1) + d(case.b1), B, T, H, Dv)
    # prep backward: g_ln = G W1^T + g_l_ln, then the LayerNorm's backward on (mean, rstd)
    g_ln = gather_acz(d(case.g_a), d(case.g_c), d(case.g_z), B, T, H, Dv, x) @ d(case.W1).t()
    if case.g_l_ln is not None:
        g_ln = g_ln + d(case.g_l_ln).view(M, Dl)
    gw = g_ln * lw
    g_l_in = rstd * (gw - gw.mean(1, keepdim=True) - xh * (gw * xh).mean(1, keepdim=True))
    # out forward and backward
    u, colsum, gamma = d(case.u), d(case.colsum), d(case.gamma)
    scale = gamma[None, :] * _keep_rows(d(case.keep), B, T, x)
    U = rows_of_u(u / colsum[..., None], B, T, H, Dv)
    out = l_ln + scale * (d(case.o0) + U @ d(case.O))
    GU = (d(case.g).view(M, Dl) * scale) @ d(case.O).t()
    g_u = u_of_rows(GU, B, T, H, Dv) / colsum[..., None]
    g_colsum = -(g_u * u).sum(-1) / colsum
    return types.SimpleNamespace(l_ln=l_ln.view(B, T, Dl), a=a, c=c, z=z, stats=torch.cat([mean, rstd], 1), g_l_in=g_l_in.view(B, T, Dl),
                                 out=out.view(B, T, Dl), g_u=g_u, g_colsum=g_colsum)


# ---- the same as a composition of ordinary torch ops, differentiable, in the inputs' dtype ------------------------------------

def composition_prep(l_in, ln_w, ln_b, eps, W1, b1, H, Dv):
    """F.layer_norm, one addmm, and the permutes of transformer.BiMultiHeadAttention.forward -> l_ln, a, c, z."""
    B, T, Dl = l_in.shape
    HD = H * Dv
    l_ln = F.layer_norm(l_in, (Dl,), ln_w, ln_b, eps)
    P = torch.addmm(b1, l_ln.reshape(B * T, Dl), W1).view(B, T, -1)
    a = P[..., :HD].reshape(B, T, H, Dv).permute(0, 3, 2, 1).reshape(B, Dv, H * T)
    c = P[..., HD:HD + H].permute(0, 2, 1).reshape(B, H * T)
    z = P[..., HD + H:].reshape(B, T, H, Dv).permute(0, 2, 1, 3).reshape(B, H * T, Dv)
    return l_ln, a, c, z


def composition_out(u, colsum, l_ln, O, o0, gamma, keep, H):
    B, T, Dl = l_ln.shape
    Dv = u.shape[-1]
    U = (u / colsum[..., None]).view(B, H, T, Dv).permute(0, 2, 1, 3).reshape(B * T, H * Dv)
    scale = gamma if keep is None else gamma * keep.view(B, 1, 1)
    return l_ln + scale * torch.addmm(o0, U, O).view(B, T, Dl)


def composition_all(case, device=None, dtype=None):
    """The nine OUTPUTS of the composition + autograd on a case's inputs (moved to ``device`` / ``dtype`` first)."""
    to = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)
    B, T, H, Dv, Dl = case.B, case.T, case.H, case.Dv, case.Dl
    l_in = to(case.l_in).requires_grad_()
    l_ln, a, c, z = composition_prep(l_in, to(case.ln_w), to(case.ln_b), case.eps, to(case.W1), to(case.b1), H, Dv)
    loss = l_ln.sum() * 0
    for t, g in ((a, case.g_a), (c, case.g_c), (z, case.g_z), (l_ln, case.g_l_ln)):
        if g is not None:
            loss = loss + (t * to(g)).sum()
    g_l_in, = torch.autograd.grad(loss, [l_in])
    x = l_in.detach().view(B * T, Dl)
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + case.eps)
    u, colsum = to(case.u).requires_grad_(), to(case.colsum).requires_grad_()
    out = composition_out(u, colsum, l_ln.detach(), to(case.O), to(case.o0), to(case.gamma), to(case.keep), H)
    g_u, g_colsum = torch.autograd.grad((out * to(case.g)).sum(), [u, colsum])
    return types.SimpleNamespace(l_ln=l_ln.detach(), a=a.detach(), c=c.detach(), z=z.detach(), stats=torch.cat([mean, rstd], 1),
                                 g_l_in=g_l_in, out=out.detach(), g_u=g_u, g_colsum=g_colsum)


# ---- input builders -----------------------------------------------------------------------------------------------------------

def _case(shape, **kw):
    B, T, H, Dv, Dl, note = shape
    case = types.SimpleNamespace(shape=shape, B=B, T=T, H=H, Dv=Dv, Dl=Dl, eps=EPS, **kw)
    return case


def with_(case, **kw):
    """A copy of the case with some inputs replaced (None for a nullable one: a null pointer)."""
    out = types.SimpleNamespace(**case.__dict__)
    out.__dict__.update(kw)
    return out


def _keep(B, values, g):
    """[B] with entries among the two ``values``, at least one of each where B > 1 (B = 1: the second)."""
    if B == 1:
        return torch.tensor([values[1]])
    k = torch.randint(0, 2, (B,), generator=g)
    k[int(torch.randint(0, B, (1,), generator=g))] = 0
    k[(int(k.argmin()) + 1 + int(torch.randint(0, B - 1, (1,), generator=g))) % B] = 1
    return torch.tensor(values)[k]


def _seed(shape, salt):
    B, T, H, Dv, Dl, note = shape
    return ((((salt * 131 + B) * 131 + T) * 131 + H) * 131 + Dv) * 131 + Dl


def _sign(shape_, g):
    return torch.randint(0, 2, shape_, generator=g).float() * 2 - 1


def random_case(shape, gain=1.0, drop=0.3):
    """l_in = (3 N(0, 1) + 1.5) gain (a mean well above the spread); weights N(0, 0.05), biases N(0, 0.1), ln_w in [0.5, 1.5],
    gamma in +-[0.5, 1.5], u N(0, 1), colsum uniform in [0.5, 50], keep in {0, 1 / (1 - drop)}, gradients gain N(0, 1)."""
    B, T, H, Dv, Dl, note = shape
    g = torch.Generator().manual_seed(_seed(shape, 1))
    HD, N1 = H * Dv, 2 * H * Dv + H
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    return _case(
        shape, l_in=(rn(B, T, Dl) * 3 + 1.5) * gain, ln_w=0.5 + ru(Dl), ln_b=rn(Dl) * 0.1, W1=rn(Dl, N1) * 0.05, b1=rn(N1) * 0.1,
        O=rn(HD, Dl) * 0.05, o0=rn(Dl) * 0.1, gamma=(0.5 + ru(Dl)) * _sign((Dl,), g), keep=_keep(B, (0.0, 1.0 / (1.0 - drop)), g),
        u=rn(B, H * T, Dv), colsum=0.5 + 49.5 * ru(B, H * T), g_a=rn(B, Dv, H * T) * gain, g_c=rn(B, H * T) * gain,
        g_z=rn(B, H * T, Dv) * gain, g_l_ln=rn(B, T, Dl) * gain, g=rn(B, T, Dl) * gain)


def gather_row(n, Dl):
    """exact_gather_case: the row of W1 that holds the single 1.0 of column n."""
    return (7 * n + 3) % Dl


def exact_gather_case(shape):
    """The random case with W1 = one 1.0 per column n, at row gather_row(n), and b1 = 0: every entry of a, c, z is then a copy
    of the kernel's OWN l_ln[m, gather_row(n)] (0 + 1.0 x, and + 0), whatever the LayerNorm rounded to -- the row routing
    (b, t) and the column routing (h, d) show bit for bit."""
    case = random_case(shape)
    N1 = case.W1.shape[1]
    W1 = torch.zeros(case.Dl, N1)
    W1[gather_row(torch.arange(N1), case.Dl), torch.arange(N1)] = 1.0
    return with_(case, W1=W1, b1=torch.zeros(N1))


def gathered(l_ln, case):
    """What a, c, z must be on exact_gather_case given the l_ln output of the same call."""
    N1 = case.W1.shape[1]
    P = l_ln.reshape(case.B * case.T, case.Dl)[:, gather_row(torch.arange(N1, device=l_ln.device), case.Dl)]
    return scatter_acz(P, case.B, case.T, case.H, case.Dv)


def exact_integer_case(shape):
    """Inputs on which l_ln, a, c, z, out, g_u, g_colsum are exact in fp32 whatever the order of the sums: ln_w = 0 and ln_b
    integers in [-3, 3] (l_ln IS ln_b); W1, b1, O, o0 integers in [-2, 2]; u, g and the incoming gradients integers in [-4, 4];
    colsum and |gamma| in {0.5, 1, 2, 4}; keep in {0, 2}.  Scaling by a power of two is exact, and every sum of terms of one
    scale stays far below 2^24 units (exact_integer_bound; proven on the CPU).  g_l_in is 0 here (ln_w = 0) and stats depend
    on l_in: the GPU test checks the prep backward's sums on these gradients with the random case's ln_w instead."""
    B, T, H, Dv, Dl, note = shape
    g = torch.Generator().manual_seed(_seed(shape, 2))
    HD, N1 = H * Dv, 2 * H * Dv + H
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    p2 = lambda *s: torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, s, generator=g)]
    return _case(
        shape, l_in=torch.randn(B, T, Dl, generator=g) * 3 + 1.5, ln_w=torch.zeros(Dl), ln_b=ri(-3, 3, Dl), W1=ri(-2, 2, Dl, N1),
        b1=ri(-2, 2, N1), O=ri(-2, 2, HD, Dl), o0=ri(-2, 2, Dl), gamma=p2(Dl) * _sign((Dl,), g), keep=_keep(B, (0.0, 2.0), g),
        u=ri(-4, 4, B, H * T, Dv), colsum=p2(B, H * T), g_a=ri(-4, 4, B, Dv, H * T), g_c=ri(-4, 4, B, H * T),
        g_z=ri(-4, 4, B, H * T, Dv), g_l_ln=ri(-4, 4, B, T, Dl), g=ri(-4, 4, B, T, Dl))


def exact_integer_bound(case):
    """The largest sum of magnitudes that any fp32 accumulation of exact_integer_case can reach, in units of the smallest
    step of its terms (float64, from the absolute values): the prep forward's product (integers), the prep backward's
    G W1^T + g_l_ln (integers), the out forward's o0 + U O (quarters: u / colsum) and its scaled sum beside l_ln (eighths),
    the out backward's (g scale) O^T (integers: |gamma| keep is 0 or >= 1) and the colsum backward's sum over d of
    GU u (integers; the row's 1 / colsum is a common power of two)."""
    B, T, H, Dv, Dl = case.B, case.T, case.H, case.Dv, case.Dl
    M = B * T
    ab = lambda t: t.double().abs()
    lb = ab(case.ln_b).expand(M, Dl)
    prep = lb @ ab(case.W1) + ab(case.b1)
    bwd = gather_acz(ab(case.g_a), ab(case.g_c), ab(case.g_z), B, T, H, Dv, lb) @ ab(case.W1).t() + ab(case.g_l_ln).view(M, Dl)
    scale = ab(case.gamma)[None, :] * _keep_rows(ab(case.keep), B, T, lb)
    s = ab(case.o0) + rows_of_u(ab(case.u) / ab(case.colsum)[..., None], B, T, H, Dv) @ ab(case.O)
    GU = (ab(case.g).view(M, Dl) * scale) @ ab(case.O).t()
    gcs = (u_of_rows(GU, B, T, H, Dv) * ab(case.u)).sum(-1)
    return max(float(prep.max()), float(bwd.max()), 4 * float(s.max()), 8 * float((scale * s + lb).max()), float(GU.max()),
               float(gcs.max()))


def integer_g_ln(case):
    """G W1^T of exact_integer_case's gradients, exactly (float64 -> fp32; integers below 2^24): [B, T, Dl]."""
    d = lambda t: None if t is None else t.double()
    G = gather_acz(d(case.g_a), d(case.g_c), d(case.g_z), case.B, case.T, case.H, case.Dv, case.l_in.double())
    return (G @ case.W1.double().t()).float().view(case.B, case.T, case.Dl)
