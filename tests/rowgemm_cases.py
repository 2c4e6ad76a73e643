"""Cases, inputs, float64 references and error bounds for the tests of the row GEMM (csrc/rowgemm.hip, C ABI zira_rowgemm_f32),
shared by the CPU test that proves them (test_rowgemm_cases_cpu.py) and the GPU test that runs the kernel on them
(test_rowgemm_cases_gpu.py).  No GPU is needed here.

Logical rows are (query, batch): r = q * batch + b.  An operand marked batch-first lives at memory row b * Q + q; pos, res, mask
and the LayerNorm arrays are always in logical order (include/zira_msda.h)."""
import types

import torch

U = 2.0 ** -24        # unit roundoff of float32
LN_EPS = 1e-5
LNB_K = 256           # kLnbK of rowgemm.hip: the row length of the LayerNorm-backward prologue

FLAGS = ("bias", "pos", "pos_partial", "res", "mask", "relu", "ln", "ln_save", "lnb", "lnb_save", "a_batch_first", "c_batch_first")


def form(m, n, k, w_is_nk, ln, lnb):
    """(NK, BM, TW, LNB, kDepth, threads, columns_per_block) of the launch zira_rowgemm_f32 chooses.

    A MIRROR of the tiling decision at the end of the launcher in csrc/rowgemm.hip (`bm`, `narrow`, `deep` and the
    `rows * (n / 128) < 160` switch): it must be kept in step with it by hand."""
    bm = 16 if (ln or k > 1024) else 32
    rows = (m + bm - 1) // bm
    narrow = bm == 32 and not w_is_nk and rows * (n // 128) < 160
    threads = 512 if ln else 256
    cols = 256 if ln else (64 if narrow else 128)
    deep = k % 256 == 0
    if bm == 16:
        return (bool(w_is_nk), 16, 2, False, 8, threads, cols)
    if w_is_nk:
        return (True, 32, 2, bool(lnb), 8, threads, cols)
    if narrow:
        if lnb:
            return (False, 32, 1, True, 16, threads, cols)
        return (False, 32, 1, False, 16 if deep else 8, threads, cols)
    return (False, 32, 2, bool(lnb), 8, threads, cols)


# The nine instantiations the launcher can reach, as (NK, BM, TW, LNB, kDepth).
INSTANTIATIONS = {
    (True, 16, 2, False, 8), (False, 16, 2, False, 8),
    (True, 32, 2, True, 8), (True, 32, 2, False, 8),
    (False, 32, 1, True, 16), (False, 32, 1, False, 16), (False, 32, 1, False, 8),
    (False, 32, 2, True, 8), (False, 32, 2, False, 8),
}


def _call(where, n, k, rows="QB", pos_cols=None, **flags):
    """One rowgemm() call of the model: `where` = file:line, `rows` = which row count it runs at ("QB": queries x batch,
    "TB": text tokens x batch, "PIX": the pixels of one image), pos_cols = None for every column."""
    unknown = set(flags) - set(FLAGS)
    assert not unknown, unknown
    if flags.get("pos") and pos_cols is not None and pos_cols < n:
        flags["pos_partial"] = True
    return types.SimpleNamespace(where=where, n=n, k=k, rows=rows, pos_cols=pos_cols, flags=frozenset(f for f, v in flags.items() if v))


# Every rowgemm() call of decoder_layer.py and dense.py, transcribed by hand (E = 256, d_ffn = 2048, 3 * heads * levels * points
# = 384 sampling columns, 512-wide sine embedding).  All of them pass w_is_nk=False.
DECODER_CALLS = [
    _call("decoder_layer.py:148", 768, 256, bias=True, pos=True, pos_cols=512),                       # q, k, v of the self-attention
    _call("decoder_layer.py:155", 256, 256, bias=True, res=True, ln=True, ln_save=True),              # its out-projection + norm2
    _call("decoder_layer.py:157", 256, 256, bias=True, pos=True),                                     # q of the text cross-attention
    _call("decoder_layer.py:158", 512, 256, rows="TB", bias=True),                                    # its k, v from the text
    _call("decoder_layer.py:166", 256, 256, bias=True, res=True, ln=True, ln_save=True),              # its out-projection + catext_norm
    _call("decoder_layer.py:170", 384, 256, bias=True, pos=True, c_batch_first=True),                 # MSDA offsets and logits
    _call("decoder_layer.py:183", 256, 256, bias=True, res=True, ln=True, ln_save=True, a_batch_first=True),   # MSDA out-projection + norm1
    _call("decoder_layer.py:220", 2048, 256, mask=True, lnb=True, lnb_save=True),                     # norm3 gradient, W2, ReLU gradient
    _call("decoder_layer.py:224", 256, 256, lnb=True, lnb_save=True, c_batch_first=True),             # norm1 gradient, MSDA out-projection
    _call("decoder_layer.py:235", 256, 384, res=True, a_batch_first=True),                            # sampling projection's input gradient
    _call("decoder_layer.py:237", 256, 256, lnb=True, lnb_save=True),                                 # catext_norm gradient, out-projection
    _call("decoder_layer.py:250", 256, 512, rows="TB"),                                               # gradient of the text
    _call("decoder_layer.py:251", 256, 256, res=True),                                                # q projection's input gradient
    _call("decoder_layer.py:253", 256, 256, lnb=True, lnb_save=True),                                 # norm2 gradient, out-projection
    _call("decoder_layer.py:265", 256, 768, res=True),                                                # q, k, v projection's input gradient
    _call("decoder_layer.py:353", 256, 256, bias=True, relu=True),                                    # box MLP, layer 0
    _call("decoder_layer.py:354", 256, 256, bias=True, relu=True),                                    # box MLP, layer 1
    _call("decoder_layer.py:398", 256, 256, mask=True),                                               # box MLP backward through layer 1
    _call("decoder_layer.py:399", 256, 256, res=True),                                                # ... layer 0 (res = the norm's gradient)
    _call("decoder_layer.py:457", 256, 512, bias=True, relu=True),                                    # position MLP, layer 0
    _call("decoder_layer.py:458", 256, 256, bias=True),                                               # position MLP, layer 1
    _call("dense.py:361", 256, 128, rows="PIX", bias=True, res=True),                                 # fusion block's image side
]

# Row counts at which a call's form is evaluated: 900 queries x 2 images and x 1; 32 and 194 text tokens x 2; the pixels of a
# 800 x 1333 image's four levels.
ROW_COUNTS = {"QB": (1800, 900), "TB": (64, 388), "PIX": (22223,)}


def _case(name, m, n, k, nk=False, batch=0, pos_cols=None, **flags):
    unknown = set(flags) - set(FLAGS)
    assert not unknown, unknown
    if flags.get("ln"):
        flags["ln_save"] = True       # (every LayerNorm case is run with and without the saved arrays)
    if flags.get("lnb"):
        flags["lnb_save"] = True
    if flags.get("pos") and pos_cols is not None and pos_cols < n:
        flags["pos_partial"] = True
    fl = frozenset(f for f, v in flags.items() if v)
    return types.SimpleNamespace(name=name, m=m, n=n, k=k, nk=nk, batch=batch, pos_cols=pos_cols, flags=fl,
                                 form=form(m, n, k, nk, "ln" in fl, "lnb" in fl))


# Each entry is the smallest shape that reaches its form with a ragged last row block (m % BM != 0), except the pair that
# brackets the narrow switch, whose m is what the switch fixes.
CASES = [
    # <KN,16,2,plain,8>, LayerNorm epilogue: the decoder's three out-projections
    _case("kn16-ln", 21, 256, 256, bias=True, res=True, ln=True),
    _case("kn16-ln-abf", 21, 256, 256, batch=3, bias=True, res=True, ln=True, a_batch_first=True),
    # bm = 16 by K > 1024, both orientations
    _case("kn16-k1152", 17, 128, 1152),
    _case("nk16-k1152", 17, 128, 1152, nk=True),
    # <NK,16,2,plain,8> with the LayerNorm epilogue, a single prefetch round
    _case("nk16-ln-k128", 21, 256, 128, nk=True, bias=True, res=True, ln=True),
    # <NK,32,2,plain,8>
    _case("nk32-pos128", 37, 256, 128, nk=True, pos=True, pos_cols=128),
    _case("nk32-k1024", 33, 128, 1024, nk=True),                                    # 132 608 bytes of LDS: the opt-in
    # <NK,32,2,lnb,8>: in the ABI, without a caller
    _case("nk32-lnb", 37, 128, 256, nk=True, lnb=True),
    # <KN,32,1,plain,16> narrow, deep
    _case("kn32n-deep-pos128", 50, 256, 256, pos=True, pos_cols=128),               # blocks 0 and 1 of four take the code
    _case("kn32n-deep-pos", 50, 256, 256, bias=True, pos=True),
    _case("kn32n-deep-pos-cbf", 50, 384, 256, batch=2, bias=True, pos=True, c_batch_first=True),
    _case("kn32n-deep-k512-relu", 50, 256, 512, bias=True, relu=True),
    _case("kn32n-deep-bias", 35, 512, 256, bias=True),
    _case("kn32n-deep-plain", 35, 256, 512),
    _case("kn32n-deep-k768-res", 50, 256, 768, res=True),
    _case("kn32n-deep-mask", 50, 256, 256, mask=True),
    # <KN,32,1,plain,8> narrow, not deep
    _case("kn32n-k384-abf-res", 50, 256, 384, batch=2, res=True, a_batch_first=True),
    _case("kn32n-k128", 50, 256, 128, bias=True),
    # <KN,32,1,lnb,16>
    _case("kn32n-lnb-cbf", 50, 256, 256, batch=2, lnb=True, c_batch_first=True),
    _case("kn32n-lnb-cbf-mask", 50, 256, 256, batch=2, lnb=True, c_batch_first=True, mask=True),
    _case("kn32n-lnb", 50, 256, 256, lnb=True),
    # <KN,32,2,plain,8> wide
    _case("kn32w-pos512", 833, 768, 256, bias=True, pos=True, pos_cols=512),
    _case("kn32w-pos-cbf", 1701, 384, 256, batch=3, bias=True, pos=True, c_batch_first=True),
    # <KN,32,2,lnb,8> wide
    _case("kn32w-lnb-mask", 289, 2048, 256, lnb=True, mask=True),
    # both sides of the narrow switch: 159 row blocks x 1 (narrow) and 160 x 1 (wide)
    _case("switch-narrow", 5088, 128, 128, bias=True, res=True),
    _case("switch-wide", 5089, 128, 128, bias=True, res=True),
]
SWITCH_PAIR = ("switch-narrow", "switch-wide")


def case_id(c):
    return c.name


def mem_rows(m, batch):
    """perm[r] = the memory row of logical row r = q * batch + b in a batch-first tensor: b * Q + q."""
    Q = m // batch
    r = torch.arange(m)
    return (r % batch) * Q + r // batch


def inputs(c):
    """The case's operands as float32 CPU tensors, O(1) with random signs, in LOGICAL row order, plus `a_mem`: a as the kernel
    reads it (batch-first when the case says so)."""
    g = torch.Generator().manual_seed(7919 + 31 * [x.name for x in CASES].index(c.name))
    f = c.flags
    t = types.SimpleNamespace(bias=None, pos=None, res=None, mask=None, ln_gamma=None, ln_beta=None, lnb_x=None, lnb_gamma=None,
                              lnb_mean=None, lnb_rstd=None)
    t.a = torch.randn(c.m, c.k, generator=g)
    t.w = torch.randn((c.n, c.k) if c.nk else (c.k, c.n), generator=g) / c.k ** 0.5
    if "bias" in f:
        t.bias = torch.randn(c.n, generator=g)
    if "pos" in f:
        t.pos = torch.randn(c.m, c.k, generator=g)
    if "res" in f:
        t.res = torch.randn(c.m, c.n, generator=g)
    if "mask" in f:
        # a ReLU's output; where it was positive a few entries are planted that the contract `mask <= 0 -> 0` must zero
        h = torch.randn(c.m, c.n, generator=g).relu()
        live = torch.nonzero(h.reshape(-1) > 0).reshape(-1)
        pick = live[torch.randperm(live.numel(), generator=g)[:24]]
        h.reshape(-1)[pick[0::3]] = -0.0
        h.reshape(-1)[pick[1::3]] = 0.0
        h.reshape(-1)[pick[2::3]] = -1.5
        h.reshape(-1)[-1] = -0.0                                                      # the last entry of the last (ragged) block
        t.mask = h
        t.planted = torch.cat([pick, torch.tensor([c.m * c.n - 1])])
    if "ln" in f:
        t.ln_gamma = 1 + 0.1 * torch.randn(c.n, generator=g)
        t.ln_beta = 0.1 * torch.randn(c.n, generator=g)
    if "lnb" in f:
        assert c.k == LNB_K
        t.lnb_x = torch.randn(c.m, c.k, generator=g) * 2 + 0.5
        t.lnb_gamma = 1 + 0.1 * torch.randn(c.k, generator=g)
        xd = t.lnb_x.double()
        t.lnb_mean = xd.mean(-1).float()
        t.lnb_rstd = (xd.var(-1, unbiased=False) + LN_EPS).rsqrt().float()
    t.a_mem = t.a
    if "a_batch_first" in f:
        t.a_mem = torch.empty_like(t.a)
        t.a_mem[mem_rows(c.m, c.batch)] = t.a
    return t


def pos_cols(c):
    """The value of the ABI's pos_cols (the Python wrapper maps 0 to N)."""
    return c.n if c.pos_cols is None else c.pos_cols


def op_w(c, w):
    """op(W) as [K, N]."""
    return w.t() if c.nk else w


def gamma_k(k):
    """Any order of float32 sums of k + 3 rounded terms (the k products, bias, res and the rounding of the result)."""
    return (k + 3) * U / (1 - (k + 3) * U)


def product_f64(c, t, operand=None):
    """The float64 product with its elementwise float32 error bound.

    Returns (pre, bound): pre = prologue(A) @ op(W) + bias + res [m, n] in logical row order, before the mask / ReLU; bound with
    |fl(pre) - pre| <= bound for any float32 summation order.  `operand` (float32, [m, k]) replaces prologue(A): the returned
    lnb_dx of a LayerNorm-backward case, which the kernel multiplies as it stands."""
    W = op_w(c, t.w).double()
    g = gamma_k(c.k)
    if operand is not None:
        pre = operand.double() @ W
        absp = operand.double().abs() @ W.abs()
        bound = g * absp
    elif t.pos is not None:
        pc = pos_cols(c)
        ap32 = t.a + t.pos                                        # A' as the kernel forms it: one float32 rounding
        ap64 = t.a.double() + t.pos.double()
        pre = torch.cat([ap64 @ W[:, :pc], t.a.double() @ W[:, pc:]], -1)
        absp = torch.cat([ap32.double().abs() @ W[:, :pc].abs(), t.a.double().abs() @ W[:, pc:].abs()], -1)
        extra = torch.zeros_like(absp)
        extra[:, :pc] = U * (1 + g) * absp[:, :pc]                # |a + pos - A'| <= u |A'|, carried through the sum
        bound = g * absp + extra
    else:
        pre = t.a.double() @ W
        absp = t.a.double().abs() @ W.abs()
        bound = g * absp
    if t.bias is not None:
        pre = pre + t.bias.double()
        bound = bound + g * t.bias.double().abs()
    if t.res is not None:
        pre = pre + t.res.double()
        bound = bound + g * t.res.double().abs()
    return pre, bound


def activate(c, t, pre):
    """mask <= 0 -> 0, then ReLU."""
    out = pre
    if t.mask is not None:
        out = torch.where(t.mask > 0, out, torch.zeros_like(out))
    if "relu" in c.flags:
        out = torch.where(out > 0, out, torch.zeros_like(out))
    return out


def exact_zero(c, t, pre, bound):
    """Entries that must be exactly zero: masked ones, and rectified ones whose pre-activation is below zero by more than its
    bound.  Within the bound of the kink either side is right (ReLU is 1-Lipschitz: |got - relu(pre)| <= bound still holds)."""
    z = torch.zeros_like(pre, dtype=torch.bool)
    if t.mask is not None:
        z |= ~(t.mask > 0)
    if "relu" in c.flags:
        z |= pre < -bound
    return z


def kink_band(c, t, pre, bound):
    """Number of entries of a ReLU case whose pre-activation lies within its own bound of zero."""
    if "relu" not in c.flags:
        return 0
    return int((pre.abs() <= bound).sum())


def layernorm_f64(s, gamma, beta, eps=LN_EPS):
    """(y, mean, rstd) of the rows of s, written out: biased variance, y = (s - mean) rstd gamma + beta."""
    s = s.double()
    n = s.shape[-1]
    mean = s.sum(-1) / n
    d = s - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).sum(-1) / n + eps)
    y = d * rstd[:, None]
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y, mean, rstd


def layernorm_bwd_f64(dy, x, gamma, mean, rstd):
    """dx = rstd (g - mean_c g - xhat mean_c(g xhat)), g = dy gamma, xhat = (x - mean) rstd, on the statistics as given."""
    dy, x, mean, rstd = dy.double(), x.double(), mean.double(), rstd.double()
    g = dy * gamma.double() if gamma is not None else dy
    xhat = (x - mean[:, None]) * rstd[:, None]
    k = x.shape[-1]
    m1 = g.sum(-1, keepdim=True) / k
    m2 = (g * xhat).sum(-1, keepdim=True) / k
    return rstd[:, None] * (g - m1 - xhat * m2)


def to_memory(c, logical):
    """The [m, n] result as the kernel leaves it in c: memory row b * Q + q holds logical row q * batch + b when c_batch_first."""
    if "c_batch_first" not in c.flags:
        return logical
    mem = torch.empty_like(logical)
    mem[mem_rows(c.m, c.batch)] = logical
    return mem
