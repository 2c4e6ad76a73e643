"""Inputs and references for the tests of the fused bi-softmax (csrc/bisoftmax.hip), shared by the CPU test that proves the
inputs (test_bisoftmax_cases_cpu.py) and the GPU tests that run the kernels on them (test_bisoftmax_gpu.py).

Layouts as in the C ABI: xm, pv, e and their gradients [B, N, H*T], c, colsum, colmax and their gradients [B, H*T], gmax [1],
mask_l [B, T] and mask_v [B, N] with True = padded (or None)."""
import types

import torch

CLAMP = 50000.0
KTHREADS = 256        # threads of a block
TILE_FLOATS = 2048    # kTileFloats: the largest H*T, and rows per tile = TILE_FLOATS // HT clamped to [1, 64]
MAX_ROW_BLOCKS = 512  # kMaxRowBlocks, and the cap of the column-maximum chunks

# (B, N, H, T, stable, clamp_lo, clamp_hi, masked text tokens per image | None, masked image rows per image | None, note).
# The note is "<branch> | <remarks>": <branch> is what branch_name() derives for the shape from the launcher's predicates
# (test_bisoftmax_cases_cpu.py holds every note to that).  Each shape is the smallest that reaches its branch.
SHAPES = [
    (2, 117, 4, 9, 1, 1, 1, (2, 3), (5, 11), "tile G=16 vec | HT = 36: 56 rows per tile, 3 tiles, the last of 5 rows; masks differ per image"),
    (2, 70, 3, 5, 1, 1, 1, (1, 2), (0, 7), "tile G=8 scalar | HT = 15 is odd: 256 % 15 != 0 steps j and r; 64 rows per tile, 2 tiles"),
    (2, 117, 4, 9, 1, 1, 1, (3, 1), (4, 0), "tile G=16 scalar misaligned | xm and g_pv one float into a larger buffer: vec = 0 at HT % 4 == 0"),
    (1, 40000, 4, 1, 1, 1, 1, None, (1234,), "tile G=1 vec strided colmax-rows=79 | HT = 4, j_step = 0; 625 tiles > 512 blocks; N > 32768: 512 "
                                             "column-maximum chunks of 79 rows (a thread walks 2); the fold joins 16 partials per phase"),
    (1, 20, 4, 33, 1, 1, 1, (5,), None, "tile G=64 vec | T = 33: 31 idle lanes per group; 15 rows per tile, 2 tiles; null mask_v"),
    (1, 20, 2, 64, 1, 1, 1, (1,), (3,), "tile G=64 vec | T = 64: the last T of the lane-group form"),
    (1, 20, 3, 32, 1, 1, 1, None, (2,), "tile G=32 vec | T = 32 but HT = 96: not the register form; null mask_l"),
    (2, 37, 2, 32, 1, 1, 1, (3, 0), (4, 9), "t32<1> | 2 blocks = 8 waves x U = 4 rows: a second, ragged pass with clamped loads"),
    (2, 37, 4, 32, 1, 1, 1, (0, 7), (6, 0), "t32<2> | the model's own H and T; 3 blocks, one ragged pass"),
    (1, 37, 8, 32, 1, 1, 1, (2,), (5,), "t32<4> | HT = 256, 5 blocks"),
    (2, 9, 1, 65, 1, 1, 1, (1, 4), (2, 0), "wave KPL=4 | HT = 65: column 64 alone in lane 0's second slot (H = 1: the head map cannot go wrong)"),
    (1, 2051, 1, 65, 1, 1, 1, None, (100,), "wave KPL=4 strided | N > 4 * 512: the row loop strides"),
    (1, 9, 2, 128, 1, 1, 1, (9,), (1,), "wave KPL=4 | HT = 256: the last of KPL = 4"),
    (1, 9, 1, 257, 1, 1, 1, (20,), (2,), "wave KPL=8 | HT = 257: the first of KPL = 8"),
    (1, 9, 4, 161, 1, 1, 1, None, (3,), "wave KPL=12 | HT = 644"),
    (2, 9, 4, 194, 1, 1, 1, (30, 5), (2, 4), "wave KPL=13 | HT = 776: the COCO caption; masks on both sides"),
    (1, 9, 4, 209, 1, 1, 1, (7,), (1,), "wave KPL=16 | HT = 836: the first of KPL = 16 (13 x 64 = 832 columns would lose four)"),
    (1, 9, 4, 256, 1, 1, 1, (40,), (2,), "wave KPL=16 | HT = 1024: the last wave shape"),
    (1, 6, 8, 129, 1, 1, 1, (11,), (1,), "walk vec | HT = 1032: the first shape past the wave form; one row per tile"),
    (1, 515, 16, 128, 1, 1, 1, (3,), (17,), "walk vec strided | HT = 2048, the maximum; 515 tiles of one row > 512 blocks"),
    (2, 37, 4, 9, 0, 1, 1, (2, 1), (3, 5), "tile G=16 vec | stable = 0: only then can clamp_hi bind"),
    (1, 9, 4, 70, 0, 1, 1, (6,), (2,), "wave KPL=8 | stable = 0"),
    (2, 37, 4, 9, 1, 0, 0, (1, 2), (0, 4), "tile G=16 vec | stable = 1, both clamps off"),
    (1, 9, 4, 70, 1, 0, 0, (5,), (1,), "wave KPL=8 | stable = 1, both clamps off"),
]

# clamp_case runs at these: the lane-group form, the register form (forward) and the wave form with stable = 1 (clamp_lo binds),
# the lane-group and the wave form with stable = 0 (clamp_hi binds too), and the walk.
CLAMP_SHAPES = [
    (2, 37, 4, 9, 1, 1, 1, (2, 1), (3, 5), "tile G=16 vec | clamp_lo under the global shift"),
    (1, 37, 4, 32, 1, 1, 1, (4,), (5,), "t32<2> | clamp_lo under the global shift"),
    (1, 9, 4, 70, 1, 1, 1, (6,), (2,), "wave KPL=8 | clamp_lo under the global shift"),
    (1, 6, 8, 129, 1, 1, 1, (11,), (1,), "walk vec | clamp_lo under the global shift"),
    (2, 37, 4, 9, 0, 1, 1, (2, 1), (3, 5), "tile G=16 vec | stable = 0: clamp_hi and clamp_lo"),
    (1, 9, 4, 70, 0, 1, 1, (6,), (2,), "wave KPL=8 | stable = 0: clamp_hi and clamp_lo"),
]

# the fully-masked conventions: two images in the lane-group form, the register form, the wave form and the walk
CONVENTION_SHAPES = [
    (2, 37, 4, 9, 1, 1, 1, (2, 1), (3, 5), "tile G=16 vec | two images"),
    (2, 37, 4, 32, 1, 1, 1, (0, 7), (6, 0), "t32<2> | two images"),
    (2, 9, 4, 194, 1, 1, 1, (30, 5), (2, 4), "wave KPL=13 | two images"),
    (2, 6, 8, 129, 1, 1, 1, (11, 3), (1, 0), "walk vec | two images"),
]


def shape_id(shape):
    B, N, H, T, stable, lo, hi, mtext, mrows, note = shape
    return "B%d-N%d-H%d-T%d-s%d%d%d-%s" % (B, N, H, T, stable, lo, hi, note.split(" | ")[0].replace(" ", "_"))


def misaligned(shape):
    return "misaligned" in shape[9].split(" | ")[0]


def dispatch(N, H, T, aligned=True):
    """The launchers' choices for a shape, restated from csrc/bisoftmax.hip (zira_bisoftmax_{fwd,bwd}_f32 and the helpers
    above them).  None when H*T is refused."""
    HT = H * T
    if HT > TILE_FLOATS:
        return None
    rows_per_tile = min(max(TILE_FLOATS // HT, 1), 64)
    tiles = -(-N // rows_per_tile)
    colmax_chunks = min(max(-(-N // 64), 1), MAX_ROW_BLOCKS)
    d = types.SimpleNamespace(HT=HT, rows_per_tile=rows_per_tile, tiles=tiles, colmax_chunks=colmax_chunks,
                              colmax_rows=-(-N // colmax_chunks), kpl=None, G=None, vec=None)
    if T > 64 and HT <= 1024:            # use_wave_rows: forward and backward
        d.fwd = d.bwd = "wave"
        d.kpl = 4 if HT <= 256 else 8 if HT <= 512 else 12 if HT <= 768 else 13 if HT <= 832 else 16
        d.row_blocks = min(-(-N // (KTHREADS // 64)), MAX_ROW_BLOCKS)
        d.strided = N > (KTHREADS // 64) * d.row_blocks
    else:
        d.fwd = "t32" if T == 32 and HT in (64, 128, 256) else "tile"      # (the backward of T = 32 is the tile kernel)
        d.bwd = "tile"
        d.G = 0 if T > 64 else next(g for g in (1, 2, 4, 8, 16, 32, 64) if g >= T)   # 0: one thread walks a (row, head)
        d.vec = int(HT % 4 == 0 and aligned)
        d.row_blocks = min(tiles, MAX_ROW_BLOCKS)
        d.strided = tiles > d.row_blocks
    d.workspace_floats = lambda B: B * max(d.row_blocks, colmax_chunks) * HT + B * HT + 8
    return d


def branch_name(shape):
    """The first part of a shape's note, derived from dispatch()."""
    B, N, H, T = shape[:4]
    d = dispatch(N, H, T, aligned=not misaligned(shape))
    if d.fwd == "wave":
        name = "wave KPL=%d" % d.kpl
    elif d.fwd == "t32":
        name = "t32<%d>" % (d.HT // 64)
    else:
        name = ("walk" if d.G == 0 else "tile G=%d" % d.G) + (" vec" if d.vec else " scalar")
    if misaligned(shape):
        name += " misaligned"
    if d.strided:
        name += " strided"
    if d.colmax_rows > 64:
        name += " colmax-rows=%d" % d.colmax_rows
    return name


def masks(shape):
    """mask_l [B, T], mask_v [B, N] (bool, True = padded; None where the shape has none): scattered tokens and rows, the
    counts of the shape, the same for every case of the shape."""
    B, N, H, T, stable, lo, hi, mtext, mrows, note = shape
    g = torch.Generator().manual_seed(7919 * N + 31 * T + H)
    ml = mv = None
    if mtext is not None:
        assert len(mtext) == B and all(0 <= k < T for k in mtext)
        ml = torch.zeros(B, T, dtype=torch.bool)
        for b, k in enumerate(mtext):
            ml[b, torch.randperm(T, generator=g)[:k]] = True
    if mrows is not None:
        assert len(mrows) == B and all(0 <= k < N for k in mrows)
        mv = torch.zeros(B, N, dtype=torch.bool)
        for b, k in enumerate(mrows):
            mv[b, torch.randperm(N, generator=g)[:k]] = True
    return ml, mv


def _clamp(x, clamp_lo, clamp_hi):
    if clamp_lo or clamp_hi:
        return torch.clamp(x, min=-CLAMP if clamp_lo else None, max=CLAMP if clamp_hi else None)
    return x


def reference_f64(xm, c, mask_l, mask_v, H, T, stable, clamp_lo, clamp_hi, g_pv, g_e, g_colsum):
    """The bi-softmax and its gradients written out in float64 (no autograd):

        x = xm + c;  g = max(x) if stable else 0;  x1 = clamp(x - g);  pv = softmax_t(x1) over the live text tokens;
        cm1 = max_n x1;  e = exp(clamp(x1 - cm1)), 0 on mask_v rows;  colsum = sum_n e;  colmax = max_n x;  gmax = max(x)

    Both maxima run over every entry, padded ones included.  gmax is max(x) whatever `stable` is (what the kernel writes;
    with stable = 0 the shift is 0 and nothing reads gmax).
    g_xm, g_c: the gradients of <g_pv, pv> + <g_e, e> + <g_colsum, colsum> with BOTH maxima held constant; a clamp passes
    the gradient where its input lies within [-50000, 50000], bounds included (torch.clamp).
    Conventions: a (b, n, h) whose text tokens are all masked has pv = 0 -- no NaN -- and gets nothing through g_pv; an image
    whose tokens are all masked has e = 0 and colsum = 0.
    Returns a namespace: pv, e, g_xm [B, N, H*T], colsum, colmax, g_c [B, H*T], gmax [1]."""
    B, N, HT = xm.shape
    assert HT == H * T
    inf = float("inf")
    lo, hi = (-CLAMP if clamp_lo else -inf), (CLAMP if clamp_hi else inf)
    x = xm.detach().double().view(B, N, H, T) + c.detach().double().view(B, 1, H, T)
    gmax = x.max()
    xs = x - (gmax if stable else 0.0)
    pass1 = (xs >= lo) & (xs <= hi)
    x1 = xs.clamp(lo, hi)
    xl = x1 if mask_l is None else x1.masked_fill(mask_l.bool().view(B, 1, 1, T), -inf)
    m = xl.amax(-1, keepdim=True)
    any_live = m > -inf
    ex = torch.exp(xl - torch.where(any_live, m, torch.zeros_like(m)))          # (exp(-inf) = 0)
    den = ex.sum(-1, keepdim=True)
    pv = torch.where(any_live, ex / torch.where(any_live, den, torch.ones_like(den)), torch.zeros_like(ex))
    d2 = x1 - x1.amax(1, keepdim=True)
    pass2 = (d2 >= lo) & (d2 <= hi)
    e = torch.exp(d2.clamp(lo, hi))
    if mask_v is not None:
        e = e.masked_fill(mask_v.bool().view(B, N, 1, 1), 0.0)
    gp = g_pv.detach().double().view(B, N, H, T)
    gx = pv * (gp - (gp * pv).sum(-1, keepdim=True))
    gl = (g_e.detach().double().view(B, N, H, T) + g_colsum.detach().double().view(B, 1, H, T)) * e
    gx = torch.where(pass1, gx + torch.where(pass2, gl, torch.zeros_like(gl)), torch.zeros_like(gx))
    return types.SimpleNamespace(pv=pv.reshape(B, N, HT), e=e.reshape(B, N, HT), colsum=e.sum(1).reshape(B, HT),
                                 colmax=x.amax(1).reshape(B, HT), gmax=gmax.reshape(1), g_xm=gx.reshape(B, N, HT),
                                 g_c=gx.sum(1).reshape(B, HT))


def composition(xm, c, mask_l, mask_v, H, T, stable, clamp_lo, clamp_hi, detach_maxima=True):
    """The same chain in the inputs' own dtype, differentiable: what the kernel replaces (transformer.py: _SubtractGlobalMax,
    _clamp, masked_fill + softmax over the text tokens, the column maximum, _clamp, masked_fill + exp over the image
    tokens).  The maxima are detached unless ``detach_maxima`` is False.  An image whose text tokens are all masked gets
    pv = 0 (the convention of reference_f64).  Returns pv, e, colsum, colmax, gmax."""
    B, N, HT = xm.shape
    det = (lambda t: t.detach()) if detach_maxima else (lambda t: t)
    x = xm.view(B, N, H, T) + c.view(B, 1, H, T)
    gmax = det(x).max()
    x1 = _clamp(x - gmax if stable else x, clamp_lo, clamp_hi)
    if mask_l is not None:
        ml = mask_l.bool()
        dead = ml.all(1)
        pv = x1.masked_fill((ml & ~dead[:, None]).view(B, 1, 1, T), float("-inf")).softmax(-1)
        pv = pv.masked_fill(dead.view(B, 1, 1, 1), 0.0)
    else:
        pv = x1.softmax(-1)
    e = torch.exp(_clamp(x1 - det(x1).amax(1, keepdim=True), clamp_lo, clamp_hi))
    if mask_v is not None:
        e = e.masked_fill(mask_v.bool().view(B, N, 1, 1), 0.0)
    return pv.reshape(B, N, HT), e.reshape(B, N, HT), e.sum(1).reshape(B, HT), x.detach().amax(1).reshape(B, HT), gmax.detach().reshape(1)


OUTPUTS = ("pv", "e", "colsum", "colmax", "gmax", "g_xm", "g_c")


def composition_all(case, device=None, dtype=None):
    """The seven outputs of composition() + autograd on a case's inputs (moved to ``device`` / ``dtype`` first)."""
    mv = lambda t: None if t is None else t.to(device=device)
    to = lambda t: t.to(device=device, dtype=dtype)
    xm, c = to(case.xm).requires_grad_(), to(case.c).requires_grad_()
    pv, e, colsum, colmax, gmax = composition(xm, c, mv(case.mask_l), mv(case.mask_v), case.H, case.T, case.stable, case.clamp_lo,
                                              case.clamp_hi)
    loss = (pv * to(case.g_pv)).sum() + (e * to(case.g_e)).sum() + (colsum * to(case.g_colsum)).sum()
    g_xm, g_c = torch.autograd.grad(loss, [xm, c])
    return types.SimpleNamespace(pv=pv.detach(), e=e.detach(), colsum=colsum.detach(), colmax=colmax, gmax=gmax, g_xm=g_xm, g_c=g_c)


def reference_all(case, device=None):
    mv = lambda t: None if t is None else t.to(device=device)
    return reference_f64(mv(case.xm), mv(case.c), mv(case.mask_l), mv(case.mask_v), case.H, case.T, case.stable, case.clamp_lo,
                         case.clamp_hi, mv(case.g_pv), mv(case.g_e), mv(case.g_colsum))


def _case(shape, **kw):
    B, N, H, T, stable, lo, hi, mtext, mrows, note = shape
    ml, mv = masks(shape)
    return types.SimpleNamespace(shape=shape, B=B, N=N, H=H, T=T, stable=stable, clamp_lo=lo, clamp_hi=hi, mask_l=ml, mask_v=mv, **kw)


def select(b, n, h, nlive):
    """exact_case: the index among image b's live text tokens that (n, h) selects.  Odd rows walk through all of them; even
    rows stay among the first three, so that heads h >= 1 often select a token t < h -- the columns j = h T + t that a
    head map j / (T + 1) would hand to head h - 1."""
    return torch.where(n % 2 == 1, (7 * n + 3 * h + 5 * b + n // 11) % nlive, (n // 2 + h + b) % min(nlive, 3))


def exact_case(shape, seed):
    """Inputs on which every output is exact in fp32 whatever the order of the sums.

    xm[b, n, h, t] = 0 where t is the live token that (b, n, h) selects, else -128; c holds integers in [-3, 3] (3 at the
    token that (0, 0, 0) selects: gmax = 3); g_pv, g_e, g_colsum hold integers in [-4, 4].  Every x1 difference inside a group
    and inside a column is then 0 or at most -122, and exp(-122) is 0 in fp32: pv is one-hot; e is 1 where the row selects
    the column and 0 elsewhere -- and 1 on every row of a column that no row selects (masked text tokens among them) --, 0
    on masked rows; colsum is a count (0 for a column that only masked rows select: they still set its maximum); colmax
    is c or c - 128; the softmax term of the gradient is 0 x integer, so g_xm = (g_e + g_colsum) e, and g_c its column
    sums: integers below 8 N <= 2^19.
    Returns the inputs and, as ``want``, the exact outputs (fp32)."""
    B, N, H, T = shape[:4]
    g = torch.Generator().manual_seed(seed)
    case = _case(shape)
    HT = H * T
    c = torch.randint(-3, 4, (B, H, T), generator=g).float()
    n, h = torch.arange(N)[:, None], torch.arange(H)[None, :]
    onehot = torch.zeros(B, N, H, T, dtype=torch.bool)
    for b in range(B):
        live = torch.arange(T) if case.mask_l is None else torch.nonzero(~case.mask_l[b]).flatten()
        onehot[b].scatter_(2, live[select(b, n, h, live.numel())][..., None], True)
    c[0, 0, int(onehot[0, 0, 0].nonzero())] = 3.0
    xm = torch.where(onehot, 0.0, -128.0)
    g_pv = torch.randint(-4, 5, (B, N, HT), generator=g).float()
    g_e = torch.randint(-4, 5, (B, N, HT), generator=g).float()
    g_colsum = torch.randint(-4, 5, (B, HT), generator=g).float()
    selected = onehot.any(1, keepdim=True)                                   # by any row, masked ones included
    e = torch.where(selected, onehot, torch.ones_like(onehot)).float()
    if case.mask_v is not None:
        e = e.masked_fill(case.mask_v.view(B, N, 1, 1), 0.0)
    e = e.reshape(B, N, HT)
    g_xm = (g_e + g_colsum[:, None]) * e
    case.__dict__.update(xm=xm.reshape(B, N, HT), c=c.reshape(B, HT), g_pv=g_pv, g_e=g_e, g_colsum=g_colsum)
    case.want = types.SimpleNamespace(
        pv=onehot.float().reshape(B, N, HT), e=e, colsum=e.double().sum(1).float(),
        colmax=torch.where(selected[:, 0], c, c - 128.0).reshape(B, HT), gmax=torch.tensor([3.0]), g_xm=g_xm,
        g_c=g_xm.double().sum(1).float())
    return case


def randn_case(shape, seed, gain=1.0):
    """xm = gain N(0, 1), c = N(0, 1), N(0, 1) upstream gradients (gain 8: peaked softmaxes, like the model's)."""
    B, N, H, T = shape[:4]
    g = torch.Generator().manual_seed(seed)
    HT = H * T
    return _case(shape, xm=torch.randn(B, N, HT, generator=g) * gain, c=torch.randn(B, HT, generator=g),
                 g_pv=torch.randn(B, N, HT, generator=g), g_e=torch.randn(B, N, HT, generator=g),
                 g_colsum=torch.randn(B, HT, generator=g))


def clamp_case(shape, seed):
    """Inputs on which the first clamp can be seen, forward and backward.  Every value is a multiple of 1/8 below 2^17, so
    xm + c - g is exact in fp32 and sits on, inside or outside +-50000 exactly as written here.

    Ordinary (b, n, h) groups hold xm in [-4, 4] and c in [-2, 2]; with group number i = (b N + n) H + h, i % 7 picks:
      stable = 1   1: "below" -- xm = -60000 - 8 t, distinct values that all clip to -50000: pv must be exactly uniform
                      over the live tokens and g_xm exactly 0 (without the clamp pv would be nearly one-hot; without pass1
                      g_xm would be the softmax gradient of the uniform pv);
                   3: "straddle" -- even t below, odd t ordinary;
                   5: "edge" -- t % 3 == 0 sits exactly ON -50000 after the shift (the gradient passes), the rest below:
                      uniform again, g_xm nonzero on the edge entries and 0 on the others.
      stable = 0   (g = 0)  1: "high", heads below H / 2 only -- 60000 and 70000 alternating, both clip to +50000: uniform, g_xm = 0;
                   3: "below" as above;  5: "edge high", the same heads -- even t exactly 50000, odd t 60000;
                   6: "edge low" -- even t exactly -50000, odd t below.
    (The high groups lift their columns' maxima to 50000, which zeroes e on every other row of those heads: the other
    heads keep ordinary e.)
    The second clamp cannot be seen: x1 - cm1 <= 0 by construction, and where it falls below -50000, exp(-50000) = 0 with
    or without the clamp, forward and backward (the gradient is multiplied by that e).
    Returns the case with ``uniform`` [B, N, H] (groups whose live pv must all be equal), ``clipped`` [B, N, H*T] (g_xm
    must be exactly 0) and ``edge`` [B, N, H*T] (live entries exactly on a bound: g_xm must not be 0)."""
    B, N, H, T, stable, lo, hi = shape[:7]
    assert lo and (stable or hi) and T >= 4
    g = torch.Generator().manual_seed(seed)
    case = _case(shape)
    HT = H * T
    xm = torch.randint(-32, 33, (B, N, H, T), generator=g).float() / 8
    c = torch.randint(-16, 17, (B, 1, H, T), generator=g).float() / 8
    kind = (torch.arange(B * N * H).view(B, N, H) % 7)[..., None].expand(B, N, H, T)
    low_head = (torch.arange(H) < max(1, H // 2)).view(1, 1, H, 1)
    t = torch.arange(T).view(1, 1, 1, T).expand(B, N, H, T)
    below = -60000.0 - 8.0 * t
    if stable:
        on_edge = (kind == 5) & (t % 3 == 0)
        xm = torch.where((kind == 1) | ((kind == 3) & (t % 2 == 0)) | (kind == 5), below, xm)
        gshift = (xm + c).max()                                               # (an ordinary entry: the edge entries stay below it)
        xm = torch.where(on_edge, -CLAMP + gshift - c, xm)
        uniform = (kind == 1) | (kind == 5)
    else:
        gshift = torch.tensor(0.0)
        high, edge_hi = (kind == 1) & low_head, (kind == 5) & low_head
        on_edge = (edge_hi | (kind == 6)) & (t % 2 == 0)
        xm = torch.where(high, torch.where(t % 2 == 0, 60000.0, 70000.0), xm)
        xm = torch.where((kind == 3) | (kind == 6), below, xm)
        xm = torch.where(edge_hi, 60000.0 + 0 * xm, xm)
        xm = torch.where(on_edge, torch.where(kind == 6, -CLAMP, CLAMP) - c, xm)
        uniform = high | (kind == 3) | edge_hi | (kind == 6)
    xs = (xm + c) - gshift                                                    # exact in fp32
    assert float((xm * 8).frac().abs().max()) == 0.0 and float(xm.abs().max()) < 2.0 ** 17
    assert not stable or float((xm + c).max()) == float(gshift)
    assert bool((xs[on_edge].abs() == CLAMP).all())
    clipped = (xs < -CLAMP) | ((xs > CLAMP) if hi else torch.zeros_like(on_edge))
    live = torch.ones(B, 1, 1, T, dtype=torch.bool) if case.mask_l is None else ~case.mask_l.view(B, 1, 1, T)
    case.__dict__.update(xm=xm.reshape(B, N, HT), c=c.reshape(B, HT), g_pv=torch.randn(B, N, HT, generator=g),
                         g_e=torch.randn(B, N, HT, generator=g), g_colsum=torch.randn(B, HT, generator=g),
                         uniform=uniform[..., 0].clone(), clipped=clipped.reshape(B, N, HT), edge=(on_edge & live).reshape(B, N, HT))
    return case


def fully_masked(case, text_image=None, rows_image=None):
    """The case with every text token (``text_image``) or every image token (``rows_image``) of one image masked."""
    out = types.SimpleNamespace(**case.__dict__)
    if text_image is not None:
        out.mask_l = torch.zeros(case.B, case.T, dtype=torch.bool) if case.mask_l is None else case.mask_l.clone()
        out.mask_l[text_image] = True
    if rows_image is not None:
        out.mask_v = torch.zeros(case.B, case.N, dtype=torch.bool) if case.mask_v is None else case.mask_v.clone()
        out.mask_v[rows_image] = True
    return out
