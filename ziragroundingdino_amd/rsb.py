"""ZiRa's reparameterizable dual side branch (RSB) -- ``RepZeroLinear`` / ``RepZeroConv2d``.

Mirror of the reference modules (groundingdino/models/GroundingDINO/
groundingdino_dual_zero_rep_branch.py:62-135): same constructor arguments, same parameter /
state-dict names (``weight, bias, scaling, freeze_linear.* / freeze_conv.*``), same
``forward -> (output, zero_interference_loss)`` contract and same ``__rep__`` merge.

    train: branch = scaling * F(x; W, b);  out = branch + F(x; W_f, b_f)
           loss   = mean(smooth_l1(branch, 0)) + mean(smooth_l1(out, 0))
    eval : out = F(x; W_f, b_f);  loss = zeros(1)
    __rep__ (after every task): W_f += scaling*W; b_f += scaling*b; scaling <- init; W, b <- 1e-8

The two dense contractions go to the GEMM / convolution libraries (MFMA); everything after
them -- scale, add, both SmoothL1-to-zero means, and in the backward all three gradients --
is one pass in the HIP kernels of csrc/rsb.hip (C ABI ``zira_rsb_fwd_f32 / zira_rsb_bwd_f32``).
On GPU tensors that kernel path is the only one (it raises if the extension is missing); CPU
tensors evaluate the defining expression with torch ops, as the reference does.

``RepZeroLoRA`` is the low-rank form of the language branch (reference models/GroundingDINO/adapter.py:227-259), the
alternative the dual-branch class names for ``rep_linear_adapter``: ``branch = scaling * up(down(x))`` with a ``down_dim``-wide
intermediate, no biases, the same loss and the same merge (``freeze_linear.weight += scaling * up.weight @ down.weight``).
``lora_reference`` is its train-mode definition in torch ops; ``lora_apply`` is the entry point: one autograd node,
``_LoRANative``, over the HIP kernels of csrc/lora.hip (C ABI in include/zira_lora.h) where they serve -- fp32 CUDA tensors
outside autocast, ``in_features`` a multiple of 32 up to 1024, ``down_dim`` a multiple of 32 up to 256, ``out_features`` 256, at
most 64 x 256 rows -- under ``transformer.Switches.native_lora``; everything else (CPU tensors, other dtypes, autocast, shapes
the header declines, ``FORCE_LORA_REFERENCE``) is ``lora_reference``.
"""
import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .dense import _scratch, _zeroed_once, conv2d_as_gemm, conv2d_pair_as_gemm

zero_value = 1e-8
lan_scale = 0.1
vis_scale = 0.1
FORCE_LORA_REFERENCE = False      # True: every lora_apply call is lora_reference
LORA_MAX_E, LORA_MAX_R, LORA_OUT, LORA_MAX_ROWS = (_lib.LORA_CONSTANTS["ZIRA_LORA_" + k] for k in ("MAX_E", "MAX_R", "OUT", "MAX_ROWS"))
_LORA_WS = {}
_LORA_TICKETS = {}


class _RSBEpilogue(Function):
    """(y_branch, y_twin, scaling) -> (out, loss) on the GPU through the C ABI."""

    @staticmethod
    def forward(ctx, y_branch, y_twin, scaling):
        lib = _lib.load()
        y_branch = y_branch.contiguous()
        y_twin = y_twin.contiguous()
        n = y_branch.numel()
        out = torch.empty_like(y_branch)
        loss = torch.empty(1, dtype=torch.float32, device=y_branch.device)
        ws = torch.empty(int(lib.zira_rsb_workspace_floats(n)), dtype=torch.float32,
                         device=y_branch.device)
        with torch.cuda.device(y_branch.device):
            rc = lib.zira_rsb_fwd_f32(y_branch.data_ptr(), y_twin.data_ptr(), scaling.data_ptr(), n,
                                      out.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_rsb_fwd_f32 failed: hipError %d" % rc)
        ctx.save_for_backward(y_branch, y_twin, scaling)
        return out, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_loss):
        y_branch, y_twin, scaling = ctx.saved_tensors
        lib = _lib.load()
        n = y_branch.numel()
        g_branch = torch.empty_like(y_branch)
        g_twin = torch.empty_like(y_twin)
        g_scaling = torch.empty(1, dtype=torch.float32, device=y_branch.device)
        ws = torch.empty(int(lib.zira_rsb_workspace_floats(n)), dtype=torch.float32,
                         device=y_branch.device)
        go = grad_out.contiguous() if grad_out is not None else None
        gl = grad_loss.contiguous() if grad_loss is not None else None
        with torch.cuda.device(y_branch.device):
            rc = lib.zira_rsb_bwd_f32(y_branch.data_ptr(), y_twin.data_ptr(), scaling.data_ptr(),
                                      go.data_ptr() if go is not None else None,
                                      gl.data_ptr() if gl is not None else None, n,
                                      g_branch.data_ptr(), g_twin.data_ptr(), g_scaling.data_ptr(),
                                      ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_rsb_bwd_f32 failed: hipError %d" % rc)
        return g_branch, g_twin, g_scaling.to(scaling.dtype)


def rsb_epilogue(y_branch: Tensor, y_twin: Tensor, scaling: Tensor):
    """out = scaling*y_branch + y_twin and the zero-interference loss (0-dim, as the reference)."""
    if y_branch.is_cuda:
        dt = y_branch.dtype
        out, loss = _RSBEpilogue.apply(y_branch.float(), y_twin.float(), scaling.float())
        return out.to(dt), loss.reshape(())
    branch = scaling * y_branch
    out = branch + y_twin
    loss = (F.smooth_l1_loss(branch, torch.zeros_like(branch)) +
            F.smooth_l1_loss(out, torch.zeros_like(out)))
    return out, loss


class RepZeroConv2d(nn.Conv2d):
    """Vision side branch beside an ``input_proj`` conv (reference :66-103)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0,
                 dilation=1, groups: int = 1, bias: bool = True, padding_mode: str = "zeros",
                 device=None, dtype=None, zero_value=zero_value) -> None:
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                         bias, padding_mode, device, dtype)
        self.scaling = nn.Parameter(torch.ones(1) * vis_scale)
        nn.init.constant_(self.weight, val=zero_value)
        if self.bias is not None:
            nn.init.constant_(self.bias, val=zero_value)
        self.freeze_conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding,
                                     dilation, groups, bias, padding_mode, device, dtype)
        nn.init.constant_(self.freeze_conv.weight, val=0.0)
        if self.bias is not None:
            nn.init.constant_(self.freeze_conv.bias, val=0.0)

    def _gemm_ok(self):
        return (self.dilation == (1, 1) and self.groups == 1 and self.padding_mode == "zeros"
                and not isinstance(self.padding, str))

    def forward(self, input: Tensor):
        if not self._gemm_ok():  # configurations the hot path never uses: plain conv modules
            if not self.training:
                return self.freeze_conv(input), input.new_zeros(1)
            return rsb_epilogue(super().forward(input), self.freeze_conv(input), self.scaling)
        twin = self.freeze_conv
        if not self.training:
            return conv2d_as_gemm(input, twin.weight, twin.bias, self.stride, self.padding), \
                input.new_zeros(1)
        # branch and twin read the same activations: one batched GEMM over both weight sets
        y_branch, y_twin = conv2d_pair_as_gemm(input, self.weight, self.bias, twin.weight, twin.bias,
                                               self.stride, self.padding)
        return rsb_epilogue(y_branch, y_twin, self.scaling)

    def __rep__(self):
        with torch.no_grad():
            self.freeze_conv.weight.data = self.weight.data * self.scaling + self.freeze_conv.weight.data
            self.freeze_conv.bias.data = self.bias.data * self.scaling + self.freeze_conv.bias.data
            self.scaling = nn.Parameter(torch.ones(1).to(self.weight.data) * vis_scale)
            nn.init.constant_(self.weight, val=zero_value)
            if self.bias is not None:
                nn.init.constant_(self.bias, val=zero_value)


class RepZeroLinear(nn.Linear):
    """Language side branch beside ``feat_map`` (reference :105-135).  As in the reference the
    branch *bias* keeps nn.Linear's default init at construction (only ``__rep__`` resets it)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None,
                 dtype=None) -> None:
        super().__init__(in_features, out_features, bias, device, dtype)
        self.scaling = nn.Parameter(torch.ones(1) * lan_scale)
        nn.init.constant_(self.weight, val=zero_value)
        self.freeze_linear = nn.Linear(in_features, out_features, bias, device, dtype)
        nn.init.constant_(self.freeze_linear.weight, val=0.0)
        if self.bias is not None:
            nn.init.constant_(self.freeze_linear.bias, val=0.0)

    def forward(self, input: Tensor):
        if not self.training:
            return self.freeze_linear(input), input.new_zeros(1)
        return rsb_epilogue(super().forward(input), self.freeze_linear(input), self.scaling)

    def __rep__(self):
        with torch.no_grad():
            self.freeze_linear.weight.data = self.weight.data * self.scaling + self.freeze_linear.weight.data
            self.freeze_linear.bias.data = self.bias.data * self.scaling + self.freeze_linear.bias.data
            self.scaling = nn.Parameter(torch.ones(1).to(self.weight.data) * lan_scale)
            nn.init.constant_(self.weight, val=zero_value)
            if self.bias is not None:
                nn.init.constant_(self.bias, val=zero_value)


def lora_reference(x: Tensor, w_down: Tensor, w_up: Tensor, w_twin: Tensor, scaling: Tensor):
    """The definition (``RepZeroLoRA.forward`` in training mode, adapter.py:244-250): ``branch = scaling * up(down(x))``,
    ``out = branch + freeze_linear(x)``, ``loss = mean(smooth_l1(branch, 0)) + mean(smooth_l1(out, 0))`` (beta = 1; 0-dim, every
    row counts, padding tokens included).  -> (out, loss)"""
    branch = scaling * F.linear(F.linear(x, w_down), w_up)
    out = branch + F.linear(x, w_twin)
    return out, (F.smooth_l1_loss(branch, torch.zeros_like(branch)) + F.smooth_l1_loss(out, torch.zeros_like(out)))


def _lora_tickets(dev, words):
    """The forward's ticket words on ``dev`` (``dense._zeroed_once``)."""
    return _zeroed_once(_LORA_TICKETS, dev, words, torch.int32, LORA_MAX_ROWS // 32 + 4, "rsb.lora_apply: no ticket words on %s")


def lora_native_supported(x: Tensor, w_down: Tensor, w_up: Tensor, w_twin: Tensor, scaling: Tensor) -> bool:
    """Shapes, dtypes and placement the kernels take (the switch is the caller's)."""
    if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda") and x.numel() > 0):
        return False
    R, E = w_down.shape
    if x.shape[-1] != E or tuple(w_up.shape) != (LORA_OUT, R) or tuple(w_twin.shape) != (LORA_OUT, E) or scaling.numel() != 1:
        return False
    if any(t.dtype != torch.float32 or t.device != x.device for t in (w_down, w_up, w_twin, scaling)):
        return False
    return bool(_lib.load().zira_lora_supported(x.numel() // E, E, R))


class _LoRANative(Function):
    """(x [M, E], W_down [R, E], W_up [256, R], W_twin [256, E], scaling [1]) -> (out [M, 256], loss [1]) through
    zira_lora_{fwd,bwd}_f32.  Kept for the backward: ``out`` and ``h = x W_down^T`` -- branch is formed again from h by the
    forward's instructions (the same bits), and the weight gradient of ``up`` reads h in any case."""

    @staticmethod
    def forward(ctx, x, w_down, w_up, w_twin, scaling):
        lib = _lib.load()
        x, w_down, w_up, w_twin, scaling = (t.contiguous() for t in (x, w_down, w_up, w_twin, scaling))
        M, E, R, dev = x.shape[0], x.shape[1], w_down.shape[0], x.device
        out = torch.empty((M, LORA_OUT), dtype=torch.float32, device=dev)
        h = torch.empty((M, R), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _scratch(_LORA_WS, dev, lib.zira_lora_fwd_workspace_floats(M, E, R))
            tickets = _lora_tickets(dev, lib.zira_lora_ticket_words(M))
            rc = lib.zira_lora_fwd_f32(x.data_ptr(), w_down.data_ptr(), w_up.data_ptr(), w_twin.data_ptr(), scaling.data_ptr(),
                                       M, E, R, out.data_ptr(), loss.data_ptr(), h.data_ptr(), ws.data_ptr(),
                                       tickets.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_lora_fwd_f32 failed with code %d" % rc)
        ctx.save_for_backward(x, w_down, w_up, w_twin, scaling, out, h)
        ctx.set_materialize_grads(False)
        return out, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_loss):
        x, w_down, w_up, w_twin, scaling, out, h = ctx.saved_tensors
        lib = _lib.load()
        M, E, R, dev = x.shape[0], x.shape[1], w_down.shape[0], x.device
        go = grad_out.contiguous() if grad_out is not None else None
        gl = grad_loss.reshape(1).contiguous() if grad_loss is not None else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gb, gt, gh = torch.empty_like(out), torch.empty_like(out), torch.empty_like(h)
        g_wd, g_wu, g_wt = torch.empty_like(w_down), torch.empty_like(w_up), torch.empty_like(w_twin)
        g_s = torch.empty(1, dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(dev):
            ws = _scratch(_LORA_WS, dev, lib.zira_lora_bwd_workspace_floats(M, E, R))
            rc = lib.zira_lora_bwd_f32(ptr(go), ptr(gl), x.data_ptr(), out.data_ptr(), h.data_ptr(), w_down.data_ptr(),
                                       w_up.data_ptr(), w_twin.data_ptr(), scaling.data_ptr(), M, E, R, gb.data_ptr(),
                                       gt.data_ptr(), gh.data_ptr(), ptr(gx), g_wd.data_ptr(), g_wu.data_ptr(), g_wt.data_ptr(),
                                       g_s.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_lora_bwd_f32 failed with code %d" % rc)
        return gx, g_wd, g_wu, g_wt, g_s.view(scaling.shape)


def lora_apply(x: Tensor, w_down: Tensor, w_up: Tensor, w_twin: Tensor, scaling: Tensor):
    """``(out, loss)`` of ``lora_reference`` (loss 0-dim): one autograd node over the HIP kernels where they serve, the definition
    elsewhere."""
    from .transformer import Switches

    if Switches.native_lora and not FORCE_LORA_REFERENCE and lora_native_supported(x, w_down, w_up, w_twin, scaling):
        out, loss = _LoRANative.apply(x.reshape(-1, x.shape[-1]), w_down, w_up, w_twin, scaling)
        return out.view(tuple(x.shape[:-1]) + (LORA_OUT,)), loss.reshape(())
    return lora_reference(x, w_down, w_up, w_twin, scaling)


class RepZeroLoRA(nn.Module):
    """Low-rank language side branch beside ``feat_map`` (reference adapter.py:227-259): ``down`` (in_features -> down_dim),
    ``up`` (down_dim -> out_features) and the twin ``freeze_linear``, no biases; parameter names ``scaling``,
    ``freeze_linear.weight``, ``down.weight``, ``up.weight``."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None,
                 down_dim=None) -> None:
        super().__init__()
        if bias:
            raise ValueError("RepZeroLoRA has no biases (the reference builds its three linears with bias=False)")
        self.scaling = nn.Parameter(torch.ones(1) * lan_scale)
        if down_dim is None:
            down_dim = in_features // 4
        self.freeze_linear = nn.Linear(in_features, out_features, False, device, dtype)
        self.down = nn.Linear(in_features, down_dim, False, device, dtype)
        self.up = nn.Linear(down_dim, out_features, False, device, dtype)
        nn.init.constant_(self.up.weight, val=zero_value)
        nn.init.constant_(self.down.weight, val=zero_value)
        nn.init.constant_(self.freeze_linear.weight, val=0.0)

    def forward(self, input: Tensor):
        if not self.training:
            return self.freeze_linear(input), input.new_zeros(1)
        return lora_apply(input, self.down.weight, self.up.weight, self.freeze_linear.weight, self.scaling)

    def __rep__(self):
        with torch.no_grad():
            self.freeze_linear.weight.data = ((self.up.weight.data @ self.down.weight.data) * self.scaling
                                              + self.freeze_linear.weight.data)
            self.scaling = nn.Parameter(torch.ones(1).to(self.freeze_linear.weight.data) * lan_scale)
            nn.init.constant_(self.up.weight, val=zero_value)
            nn.init.constant_(self.down.weight, val=zero_value)
