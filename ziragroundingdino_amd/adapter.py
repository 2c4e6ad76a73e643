"""The gated bottleneck ``Adapter`` of the reference's parameter-efficient baseline (models/GroundingDINO/adapter.py:124-179),
the module ``use_adapter = True`` places beside the FFN of every deformable encoder and decoder layer
(transformer_for_adapter.py:846-886, :965-1012).  ZiRa is compared against it: the same frozen detector, tuned through twelve
small adapters instead of the two side branches.  Off by default (``use_adapter = False`` in the ZiRa config).

Same parameter names (``adapter_down.{weight,bias}``, ``adapter_up.{weight,bias}``, ``gate.weight``), the same initialisation
and the same ``forward -> (output, loss)`` contract as the reference, so its checkpoints load.  ``loss`` is the reference's
"self-KD" term: the L1 mean of the adapter's INPUT (adapter.py:177 passes ``x``, not the output); kept as it is.

``adapter_reference`` is the definition in torch ops.  The hot path is one autograd node, ``_AdapterNative``, over the HIP
kernels of csrc/adapter.hip (C ABI in include/zira_adapter.h): one launch forward, the row pass, a fold and the two
tall-reduction products backward, every sum over the rows folded in a fixed order.  It serves fp32 CUDA tensors outside
autocast with D = 256, down_dim = 64, at most 8 gate rows, ReLU, and no active dropout, under
``transformer.Switches.native_adapter``; everything else -- CPU tensors, other dtypes, autocast, ``ffn_drop > 0`` in training
mode, other activations, shapes the kernels decline, ``FORCE_REFERENCE`` -- is ``adapter_reference``.

Not here: ``MoeAdapter`` (the reference's layers keep it commented out), and ``LinearAdapter``, ``TransformerAdapter`` and
``RepZeroLoRA``, which belong to model classes this package does not build.
"""
import math

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .dense import _scratch

FORCE_REFERENCE = False      # True: every call is adapter_reference
D_MODEL, DOWN_DIM, MAX_GATES = 256, 64, 8
_WS = {}
_COUNTERS = {}


def gate_scale_reference(x: Tensor, gate_weight, gate_T: float, gate_base_scale: float):
    """gate_base_scale * sigmoid(gate_T * max_g cos(x_row, gate_g)) as ``[..., 1]``, or the constant without a gate."""
    if gate_weight is None:
        return gate_base_scale
    xn = x / x.norm(dim=-1, keepdim=True)
    gn = gate_weight / gate_weight.norm(dim=-1, keepdim=True)
    max_similarity = torch.max(xn.reshape(-1, x.shape[-1]) @ gn.t(), dim=-1)[0].view(*x.shape[:-1])
    return gate_base_scale * (gate_T * max_similarity).sigmoid().unsqueeze(-1)


def adapter_reference(x: Tensor, params, activation=F.relu, dropout=None, gate_T=2.0, gate_base_scale=0.5, use_gate=True,
                      use_self_kd=True):
    """The definition (reference adapter.py:161-179).  ``params`` = (down weight, down bias, up weight, up bias, gate weight);
    ``dropout`` a callable or None.  -> (adapter_out * scale, loss [1])."""
    w_down, b_down, w_up, b_up, gate = params
    hidden = activation(F.linear(x, w_down, b_down))
    if dropout is not None:
        hidden = dropout(hidden)
    adapter_out = F.linear(hidden, w_up, b_up)
    loss = torch.zeros(1).to(x)
    if use_self_kd:
        loss = loss + x.abs().mean()      # nn.L1Loss(reduction="mean")(x, zeros_like(x))
    return adapter_out * gate_scale_reference(x, gate if use_gate else None, gate_T, gate_base_scale), loss


def _check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (name, rc))


def _counter(dev):
    """The forward's arrival counter: one zeroed word per (device, stream), which every call leaves at zero again.  While a
    stream is being captured the word comes from the graph's own pool and its clearing is part of the graph."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(4, dtype=torch.int32, device=dev)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    c = _COUNTERS.get(key)
    if c is None:
        c = _COUNTERS[key] = torch.zeros(4, dtype=torch.int32, device=dev)
    return c


def native_supported(x: Tensor, w_down, w_up, gate) -> bool:
    """Shapes, dtypes and placement the kernels take (the switches and the module's own state are the caller's)."""
    if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda") and x.numel() > 0):
        return False
    if tuple(w_down.shape) != (DOWN_DIM, D_MODEL) or tuple(w_up.shape) != (D_MODEL, DOWN_DIM) or x.shape[-1] != D_MODEL:
        return False
    if gate is not None and not (1 <= gate.shape[0] <= MAX_GATES and gate.shape[1] == D_MODEL):
        return False
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in (w_down, w_up, gate)):
        return False
    return _lib.load().zira_adapter_workspace_floats(x.numel() // D_MODEL, x.shape[-1], w_down.shape[0]) > 0


class _AdapterNative(Function):
    """(x [M, 256], W_d, b_d, W_u, b_u, gate or None) -> (y [M, 256], loss [1]) through zira_adapter_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, x, w_down, b_down, w_up, b_up, gate, gate_T, gate_base_scale, use_self_kd):
        lib = _lib.load()
        x, w_down, b_down, w_up, b_up = (t.contiguous() for t in (x, w_down, b_down, w_up, b_up))
        gate = gate.contiguous() if gate is not None else None
        M, dev = x.shape[0], x.device
        G = gate.shape[0] if gate is not None else 0
        y = torch.empty_like(x)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        h = torch.empty((M, DOWN_DIM), dtype=torch.float32, device=dev)
        rows = torch.empty((3, M), dtype=torch.float32, device=dev)       # scale, cosine, 1 / |x|
        amax = torch.empty(M, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = _scratch(_WS, dev, lib.zira_adapter_workspace_floats(M, D_MODEL, DOWN_DIM))
            _check(lib.zira_adapter_fwd_f32(x.data_ptr(), w_down.data_ptr(), b_down.data_ptr(), w_up.data_ptr(), b_up.data_ptr(),
                                            gate.data_ptr() if gate is not None else None, M, G, float(gate_T),
                                            float(gate_base_scale), int(bool(use_self_kd)), y.data_ptr(), loss.data_ptr(),
                                            h.data_ptr(), rows[0].data_ptr(), amax.data_ptr(), rows[1].data_ptr(),
                                            rows[2].data_ptr(), ws.data_ptr(), _counter(dev).data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "zira_adapter_fwd_f32")
        ctx.save_for_backward(x, w_down, w_up, b_up, gate, h, rows, amax)
        ctx.cfg = (float(gate_T), float(gate_base_scale), int(bool(use_self_kd)))
        ctx.set_materialize_grads(False)
        return y, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y, grad_loss):
        x, w_down, w_up, b_up, gate, h, rows, amax = ctx.saved_tensors
        gate_T, base, self_kd = ctx.cfg
        lib = _lib.load()
        M, dev = x.shape[0], x.device
        G = gate.shape[0] if gate is not None else 0
        gy = grad_y.contiguous() if grad_y is not None else torch.zeros_like(x)
        gl = grad_loss.reshape(1).contiguous() if grad_loss is not None else None
        gx = torch.empty_like(x)
        g_wd, g_wu = torch.empty_like(w_down), torch.empty_like(w_up)
        g_bd = torch.empty(DOWN_DIM, dtype=torch.float32, device=dev)
        g_bu = torch.empty(D_MODEL, dtype=torch.float32, device=dev)
        g_gate = torch.empty_like(gate) if gate is not None else None
        with torch.cuda.device(dev):
            ws = _scratch(_WS, dev, lib.zira_adapter_workspace_floats(M, D_MODEL, DOWN_DIM))
            _check(lib.zira_adapter_bwd_f32(gy.data_ptr(), gl.data_ptr() if gl is not None else None, x.data_ptr(), h.data_ptr(),
                                            rows[0].data_ptr(), amax.data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(),
                                            w_down.data_ptr(), w_up.data_ptr(), b_up.data_ptr(),
                                            gate.data_ptr() if gate is not None else None, M, G, gate_T, base, self_kd,
                                            gx.data_ptr(), g_wd.data_ptr(), g_bd.data_ptr(), g_wu.data_ptr(), g_bu.data_ptr(),
                                            g_gate.data_ptr() if g_gate is not None else None, ws.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "zira_adapter_bwd_f32")
        return gx, g_wd, g_bd, g_wu, g_bu, g_gate, None, None, None


class Adapter(nn.Module):
    """down (256 -> 64) -> activation -> dropout -> up (64 -> 256), scaled per row by a gate on the row's cosine to its nearest
    gate embedding (reference adapter.py:124-179).  ``forward(x [..., D]) -> (adapter_out * scale, loss [1])``."""

    def __init__(self, embed_dim=256, down_dim=64, activation=F.relu, ffn_drop=0, num_gate_embed=5, gate_T=2.0,
                 gate_base_scale=0.5, use_gate=True, use_self_kd=True, output_dim=None, **kwargs):
        super().__init__()
        if output_dim is None:
            output_dim = embed_dim
        self.adapter_down = nn.Linear(embed_dim, down_dim)
        self.adapter_relu = activation
        self.adapter_up = nn.Linear(down_dim, output_dim)
        self.dropout = nn.Dropout(p=ffn_drop)
        self.gate = nn.Embedding(num_gate_embed, embed_dim)
        self.gate_T = gate_T
        self.gate_base_scale = gate_base_scale
        self.use_gate = use_gate
        self.use_self_kd = use_self_kd
        self.output_dim = output_dim
        with torch.no_grad():
            nn.init.kaiming_uniform_(self.adapter_down.weight, a=math.sqrt(5))
            nn.init.zeros_(self.adapter_up.weight)
            nn.init.zeros_(self.adapter_down.bias)
            nn.init.zeros_(self.adapter_up.bias)

    def _params(self):
        return (self.adapter_down.weight, self.adapter_down.bias, self.adapter_up.weight, self.adapter_up.bias, self.gate.weight)

    def _native_ok(self, x: Tensor) -> bool:
        from .transformer import Switches
        relu = self.adapter_relu is F.relu or isinstance(self.adapter_relu, nn.ReLU)
        return (Switches.native_adapter and not FORCE_REFERENCE and relu and (self.dropout.p == 0 or not self.training)
                and self.output_dim == self.adapter_down.in_features
                and native_supported(x, self.adapter_down.weight, self.adapter_up.weight, self.gate.weight if self.use_gate else None))

    def forward(self, x: Tensor, **kwargs):
        if self._native_ok(x):
            w_down, b_down, w_up, b_up, gate = self._params()
            y, loss = _AdapterNative.apply(x.reshape(-1, x.shape[-1]), w_down, b_down, w_up, b_up, gate if self.use_gate else None,
                                           self.gate_T, self.gate_base_scale, self.use_self_kd)
            return y.view(x.shape), loss
        return adapter_reference(x, self._params(), self.adapter_relu, self.dropout, self.gate_T, self.gate_base_scale,
                                 self.use_gate, self.use_self_kd)
