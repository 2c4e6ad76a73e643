"""The CET text adapter of the reference's sibling class (models/GroundingDINO/groundingdino_dt.py, registry name
``dtgroundingdino``, run with ``use_cet = True``): a module beside ``feat_map`` that reads the text encoder's states (768), is
added to the projected text (``hidden_dim``) and carries a zero-interference term on its own output to zero (:182-215, :499-507).
ZiRa is compared against it, and the text-memory replay and prompt tuning were designed around it.

* ``CETAdapter`` -- ``cet_type = "Adapter"``: the reference's gated bottleneck ``Adapter`` (adapter.py:124-179) with
  ``use_self_kd = False`` and ``ffn_drop = 0``, 768 -> ``cet_middle_dim`` -> ``hidden_dim``.  Same parameter names
  (``adapter_down.{weight,bias}``, ``adapter_up.{weight,bias}``, ``gate.weight``) and the same initialisation, so a dt checkpoint's
  ``cet_adapter.*`` keys load.
* ``LinearCETAdapter`` -- ``cet_type = "Linear"``: the reference's ``LinearAdapter`` (adapter.py:7-58), one zero-initialised linear
  under the same gate.  Torch ops only.
* ``cet_type = "Transformer"`` raises ``NotImplementedError``: none of the reference's configs selects it.

``cet_reference`` is the definition in torch ops.  ``cet_apply`` is the entry point: one autograd node, ``_CETNative``, over the
HIP kernels of csrc/cet.hip (C ABI in include/zira_cet.h) where they serve -- fp32 CUDA tensors outside autocast, ``CETAdapter``
with ReLU, ``embed_dim`` a multiple of 32 up to 768, ``down_dim`` a multiple of 32 up to 1024, ``output_dim`` 256, at most 8 gate
rows, at most 64 x 256 rows -- under ``transformer.Switches.native_cet``; everything else (CPU tensors, other dtypes, autocast,
``LinearCETAdapter``, shapes the header declines, ``FORCE_REFERENCE``) is ``cet_reference``.
"""
import math

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .adapter import gate_scale_reference
from .dense import _scratch, _zeroed_once

FORCE_REFERENCE = False      # True: every call is cet_reference
CET_TYPES = ("Adapter", "Linear", "Transformer")
LOSS_CODES = {"L1": _lib.CET_CONSTANTS["ZIRA_CET_LOSS_L1"], "L2": _lib.CET_CONSTANTS["ZIRA_CET_LOSS_L2"],
              "Smooth_L1": _lib.CET_CONSTANTS["ZIRA_CET_LOSS_SMOOTH_L1"]}
LOSS_NONE = _lib.CET_CONSTANTS["ZIRA_CET_LOSS_NONE"]
MAX_E, MAX_H, OUT_DIM = (_lib.CET_CONSTANTS[k] for k in ("ZIRA_CET_MAX_E", "ZIRA_CET_MAX_H", "ZIRA_CET_OUT"))
MAX_GATES, MAX_ROWS = _lib.CET_CONSTANTS["ZIRA_CET_MAX_GATES"], _lib.CET_CONSTANTS["ZIRA_CET_MAX_ROWS"]
_WS = {}
_TICKETS = {}


def zero_loss(out: Tensor, zero_loss_type: str) -> Tensor:
    """The reference's ``adapter_loss(out, zeros_like(out))`` (:208-215): the mean ``L1Loss``, ``MSELoss`` or ``SmoothL1Loss``."""
    zeros = torch.zeros_like(out)
    if zero_loss_type == "L1":
        return F.l1_loss(out, zeros)
    if zero_loss_type == "L2":
        return F.mse_loss(out, zeros)
    if zero_loss_type == "Smooth_L1":
        return F.smooth_l1_loss(out, zeros)
    raise NotImplementedError("zero_loss_type %r: one of L1, L2, Smooth_L1" % (zero_loss_type,))


class CETAdapter(nn.Module):
    """down (embed_dim -> down_dim) -> ReLU -> up (down_dim -> output_dim), scaled per row by the gate on the row's cosine to
    its nearest gate embedding.  ``forward(x [..., embed_dim]) -> (out [..., output_dim], zeros(1))``, the reference's
    ``Adapter.forward`` with ``use_self_kd = False``."""

    def __init__(self, embed_dim, down_dim, output_dim, num_gate_embed=5, gate_T=2.0, gate_base_scale=1.0, use_gate=True):
        super().__init__()
        self.adapter_down = nn.Linear(embed_dim, down_dim)
        self.adapter_relu = F.relu
        self.adapter_up = nn.Linear(down_dim, output_dim)
        self.gate = nn.Embedding(num_gate_embed, embed_dim)
        self.gate_T, self.gate_base_scale, self.use_gate, self.output_dim = gate_T, gate_base_scale, use_gate, output_dim
        with torch.no_grad():
            nn.init.kaiming_uniform_(self.adapter_down.weight, a=math.sqrt(5))
            nn.init.zeros_(self.adapter_up.weight)
            nn.init.zeros_(self.adapter_down.bias)
            nn.init.zeros_(self.adapter_up.bias)

    def gate_scale(self, x: Tensor):
        return gate_scale_reference(x, self.gate.weight if self.use_gate else None, self.gate_T, self.gate_base_scale)

    def forward(self, x: Tensor, **kwargs):
        out = self.adapter_up(self.adapter_relu(self.adapter_down(x)))
        return out * self.gate_scale(x), torch.zeros(1).to(x)


class LinearCETAdapter(nn.Module):
    """One zero-initialised linear (embed_dim -> output_dim) under the same gate: the reference's ``LinearAdapter`` with
    ``use_self_kd = False``.  Parameter names ``linear.{weight,bias}``, ``gate.weight``."""

    def __init__(self, embed_dim, output_dim, num_gate_embed=5, gate_T=2.0, gate_base_scale=1.0, use_gate=True, **_unused):
        super().__init__()
        self.gate = nn.Embedding(num_gate_embed, embed_dim)
        self.gate_T, self.gate_base_scale, self.use_gate, self.output_dim = gate_T, gate_base_scale, use_gate, output_dim
        self.linear = nn.Linear(embed_dim, output_dim)
        with torch.no_grad():
            nn.init.zeros_(self.linear.weight)
            nn.init.zeros_(self.linear.bias)

    def gate_scale(self, x: Tensor):
        return gate_scale_reference(x, self.gate.weight if self.use_gate else None, self.gate_T, self.gate_base_scale)

    def forward(self, x: Tensor, **kwargs):
        return self.linear(x) * self.gate_scale(x), torch.zeros(1).to(x)


def build_cet_adapter(cet_type, embed_dim, cet_middle_dim, output_dim):
    """``self.cet_adapter`` of groundingdino_dt.py:182-206 (``gate_base_scale = 1.0``)."""
    if cet_type == "Adapter":
        return CETAdapter(embed_dim, cet_middle_dim, output_dim, gate_base_scale=1.0)
    if cet_type == "Linear":
        return LinearCETAdapter(embed_dim, output_dim, gate_base_scale=1.0)
    if cet_type == "Transformer":
        raise NotImplementedError('cet_type "Transformer" (the reference\'s TransformerAdapter) is not built here: none of the '
                                  "reference's configs selects it")
    raise NotImplementedError("cet_type %r: one of %s" % (cet_type, ", ".join(CET_TYPES)))


def cet_reference(x: Tensor, feat: Tensor, module, zero_loss_type="L1", use_zero_inter_loss=True):
    """The definition (groundingdino_dt.py:501-507): ``out = module(x)[0]`` -- ``up(relu(down(x))) * gate_scale(x)`` for a
    ``CETAdapter`` --, ``encoded_text = feat + out``, ``loss = zeros(1)`` plus ``L(out, 0)`` with ``use_zero_inter_loss``.
    -> (encoded_text, loss [1]).  Every row counts, padding tokens included; the mean is over all ``B * T * output_dim`` elements.

    An all-zero row does what the reference's expression does, as ``adapter.adapter_reference`` decided for the same gate:
    ``x / x.norm`` is 0 / 0, so the row's cosine, scale and output are NaN (and so is the mean); nothing special-cases it."""
    out, loss = module(x)
    if use_zero_inter_loss:
        loss = loss + zero_loss(out, zero_loss_type)
    return feat + out, loss


def _check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (name, rc))


def _tickets(dev, words):
    """The forward's ticket words on ``dev`` (``dense._zeroed_once``)."""
    return _zeroed_once(_TICKETS, dev, words, torch.int32, MAX_ROWS // 32 + 4, "cet.cet_apply: no ticket words on %s")


def native_supported(x: Tensor, feat: Tensor, module) -> bool:
    """Module kind, shapes, dtypes and placement the kernels take (the switch is the caller's)."""
    if not isinstance(module, CETAdapter) or not (module.adapter_relu is F.relu or isinstance(module.adapter_relu, nn.ReLU)):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda") and x.numel() > 0):
        return False
    w_down, w_up, gate = module.adapter_down.weight, module.adapter_up.weight, module.gate.weight if module.use_gate else None
    E, H = w_down.shape[1], w_down.shape[0]
    if x.shape[-1] != E or tuple(w_up.shape) != (OUT_DIM, H) or tuple(feat.shape) != tuple(x.shape[:-1]) + (OUT_DIM,):
        return False
    if gate is not None and not (1 <= gate.shape[0] <= MAX_GATES and gate.shape[1] == E):
        return False
    tensors = (feat, w_down, module.adapter_down.bias, w_up, module.adapter_up.bias, gate)
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in tensors):
        return False
    return bool(_lib.load().zira_cet_supported(x.numel() // E, E, H, 0 if gate is None else gate.shape[0]))


class _CETNative(Function):
    """(x [M, E], feat [M, 256], W_d, b_d, W_u, b_u, gate or None) -> (encoded_text [M, 256], loss [1]) through
    zira_cet_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, x, feat, w_down, b_down, w_up, b_up, gate, gate_T, gate_base_scale, loss_code):
        lib = _lib.load()
        x, feat, w_down, b_down, w_up, b_up = (t.contiguous() for t in (x, feat, w_down, b_down, w_up, b_up))
        gate = gate.contiguous() if gate is not None else None
        M, E, H, dev = x.shape[0], x.shape[1], w_down.shape[0], x.device
        G = gate.shape[0] if gate is not None else 0
        enc, out = torch.empty_like(feat), torch.empty_like(feat)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty((3, M), dtype=torch.float32, device=dev)       # scale, cosine, 1 / |x|
        amax = torch.empty(M, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = _scratch(_WS, dev, lib.zira_cet_fwd_workspace_floats(M, H))
            tickets = _tickets(dev, lib.zira_cet_ticket_words(M))
            _check(lib.zira_cet_fwd_f32(x.data_ptr(), feat.data_ptr(), w_down.data_ptr(), b_down.data_ptr(), w_up.data_ptr(),
                                        b_up.data_ptr(), gate.data_ptr() if gate is not None else None, M, E, H, G, float(gate_T),
                                        float(gate_base_scale), int(loss_code), enc.data_ptr(), loss.data_ptr(), out.data_ptr(),
                                        rows[0].data_ptr(), amax.data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(),
                                        ws.data_ptr(), tickets.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "zira_cet_fwd_f32")
        ctx.save_for_backward(x, w_down, b_down, w_up, gate, out, rows, amax)
        ctx.cfg = (float(gate_T), float(gate_base_scale), int(loss_code))
        ctx.set_materialize_grads(False)
        return enc, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_enc, grad_loss):
        x, w_down, b_down, w_up, gate, out, rows, amax = ctx.saved_tensors
        gate_T, base, loss_code = ctx.cfg
        lib = _lib.load()
        M, E, H, dev = x.shape[0], x.shape[1], w_down.shape[0], x.device
        G = gate.shape[0] if gate is not None else 0
        ge = grad_enc.contiguous() if grad_enc is not None else None
        gl = grad_loss.reshape(1).contiguous() if grad_loss is not None else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        h = torch.empty((M, H), dtype=torch.float32, device=dev)
        gh, gu = torch.empty_like(h), torch.empty_like(out)
        g_wd, g_wu = torch.empty_like(w_down), torch.empty_like(w_up)
        g_bd = torch.empty(H, dtype=torch.float32, device=dev)
        g_bu = torch.empty(OUT_DIM, dtype=torch.float32, device=dev)
        g_gate = torch.empty_like(gate) if gate is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(dev):
            ws = _scratch(_WS, dev, lib.zira_cet_bwd_workspace_floats(M, E, H, G))
            _check(lib.zira_cet_bwd_f32(ptr(ge), ptr(gl), x.data_ptr(), out.data_ptr(), rows[0].data_ptr(), amax.data_ptr(),
                                        rows[1].data_ptr(), rows[2].data_ptr(), w_down.data_ptr(), b_down.data_ptr(),
                                        w_up.data_ptr(), ptr(gate), M, E, H, G, gate_T, base, loss_code, h.data_ptr(),
                                        gh.data_ptr(), gu.data_ptr(), ptr(gx), g_wd.data_ptr(), g_bd.data_ptr(), g_wu.data_ptr(),
                                        g_bu.data_ptr(), ptr(g_gate), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "zira_cet_bwd_f32")
        g_feat = grad_enc if grad_enc is not None else (torch.zeros_like(out) if ctx.needs_input_grad[1] else None)
        return gx, g_feat, g_wd, g_bd, g_wu, g_bu, g_gate, None, None, None


def cet_apply(x: Tensor, feat: Tensor, module, zero_loss_type="L1", use_zero_inter_loss=True):
    """``(encoded_text, loss [1])`` of ``cet_reference``: one autograd node over the HIP kernels where they serve, the definition
    elsewhere."""
    from .transformer import Switches

    if zero_loss_type not in LOSS_CODES:
        raise NotImplementedError("zero_loss_type %r: one of L1, L2, Smooth_L1" % (zero_loss_type,))
    if Switches.native_cet and not FORCE_REFERENCE and native_supported(x, feat, module):
        E = x.shape[-1]
        enc, loss = _CETNative.apply(x.reshape(-1, E), feat.reshape(-1, OUT_DIM), module.adapter_down.weight,
                                     module.adapter_down.bias, module.adapter_up.weight, module.adapter_up.bias,
                                     module.gate.weight if module.use_gate else None, module.gate_T, module.gate_base_scale,
                                     LOSS_CODES[zero_loss_type] if use_zero_inter_loss else LOSS_NONE)
        return enc.view(feat.shape), loss
    return cet_reference(x, feat, module, zero_loss_type, use_zero_inter_loss)
