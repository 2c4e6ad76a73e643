"""The training tail on the flat gradient bucket as two launches (csrc/optim_tail.hip): L2 norm of the bucket, clip, AdamW on
every trainable tensor and the gradient clear, where the op chain is ``vector_norm``, add, divide, ``clamp``, ``mul_``, one
fused-AdamW launch per learning-rate group and ``zero_``.  The update is ``torch.optim.AdamW``'s, operation by operation in
fp32; the norm's squares are summed in double in a fixed order, so a step is a pure function of its inputs, bit for bit.

The parameters stay the separate tensors they are (state dict, derived buffers and the trainer's gradient views do not
move): the kernel reaches them through a small device table of segments -- pointer, start in the bucket, numel,
learning-rate group -- and a per-block index of the segment each fixed-size block of the flat index space begins in.  The two
moments are flat fp32 buffers laid out as the bucket.  ``export_to`` / ``import_from`` carry moments and step count to and
from a ``torch.optim.AdamW``'s ``state``, for checkpoints written through the optimizer and for changing paths mid-run.

Under fp16 loss scaling (``NativeOptimTail(..., amp=True)``, ``step_amp``) the same two launches also do the ``GradScaler``'s
part -- ``unscale_``, the skip of a step whose gradients hold an inf or a NaN, ``update`` -- on the scaler's own device tensors:
every decision is taken on the device, so the step counter lives there too and nothing is read back."""
import ctypes
import math

import torch

from . import _lib

CHUNK = _lib.CONSTANTS["ZIRA_OPTIM_TAIL_CHUNK"]        # elements of the flat index space per workgroup
MAX_GROUPS = _lib.CONSTANTS["ZIRA_OPTIM_TAIL_MAX_GROUPS"]
MAX_N = 1 << 26
_lib.assert_int64_rows(_lib.OptimSegment, ("param", "start", "numel", "group"))      # the rows NativeOptimTail uploads


def plan_segments(numels, group_ids, chunk=CHUNK):
    """Host-side planning for packed segments of the given sizes: ``(starts, block_segment)``.  ``starts[s]`` is segment s's
    offset in the bucket (back to back, no padding: the all-reduce payload is the bucket as it is); ``block_segment[b]`` is
    the segment that holds flat element ``b * chunk`` -- the first one block b touches; the kernel walks on from there while
    segments start inside the block."""
    numels, group_ids = [int(x) for x in numels], [int(g) for g in group_ids]
    assert len(numels) == len(group_ids) and len(numels) >= 1
    assert all(x >= 1 for x in numels), "an empty tensor has no place in the bucket"
    assert all(0 <= g < MAX_GROUPS for g in group_ids)
    starts, off = [], 0
    for x in numels:
        starts.append(off)
        off += x
    block_segment, s = [], 0
    for b in range((off + chunk - 1) // chunk):
        while starts[s] + numels[s] <= b * chunk:
            s += 1
        block_segment.append(s)
    return starts, block_segment


def supported(params, flat_grad) -> bool:
    """True where the native tail can serve: fp32 contiguous CUDA parameters whose ``.grad`` are, in order and back to back,
    views of the contiguous fp32 bucket ``flat_grad`` on the same device.  Anything else (CPU tensors among them) keeps the
    torch path."""
    params = list(params)
    if not params or not torch.is_tensor(flat_grad):
        return False
    if not (flat_grad.is_cuda and flat_grad.dtype == torch.float32 and flat_grad.dim() == 1 and flat_grad.is_contiguous()):
        return False
    if not 1 <= flat_grad.numel() <= MAX_N:
        return False
    off = 0
    for p in params:
        g = p.grad
        if not (p.is_cuda and p.device == flat_grad.device and p.dtype == torch.float32 and p.is_contiguous() and p.numel() >= 1):
            return False
        if g is None or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
            return False
        if g.data_ptr() != flat_grad.data_ptr() + 4 * off:
            return False
        off += p.numel()
    return off == flat_grad.numel()


class NativeOptimTail:
    """Segment table, flat moments, workspace, norm slot and the host step counter of one (parameters, bucket) binding.

    ``group_ids[i]`` is the learning-rate group of ``params[i]`` (an index into the ``lrs`` given to ``step``).  ``norm`` is
    a 0-dim fp32 device tensor that every ``step`` overwrites with the bucket's L2 norm before clipping; reading it is the
    caller's (only) synchronisation.

    ``amp=True`` adds what ``step_amp`` needs: the count of AdamW steps taken as a device int32 (a skipped step does not
    count, and only the device knows which were skipped), the 0-dim fp32 ``found_inf`` slot (0.0 or 1.0, of the latest
    ``step_amp``) and the larger workspace.  Such a tail steps through ``step_amp`` only; ``step_count`` is then the value of
    the last ``sync_step_count()``."""

    def __init__(self, params, flat_grad, group_ids, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amp=False):
        params, group_ids = list(params), [int(g) for g in group_ids]
        if not supported(params, flat_grad):
            raise RuntimeError("NativeOptimTail: these parameters / this bucket are not served (see optim_tail.supported)")
        self.params, self.flat_grad, self.group_ids = params, flat_grad, group_ids
        self.n_groups = max(group_ids) + 1
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.step_count = 0
        dev, n = flat_grad.device, flat_grad.numel()
        self.numels = [p.numel() for p in params]
        self.starts, block_segment = plan_segments(self.numels, group_ids)
        table = [[p.data_ptr(), s, x, g] for p, s, x, g in zip(params, self.starts, self.numels, group_ids)]
        self._segments = torch.tensor(table, dtype=torch.int64).to(dev)          # zira_optim_segment[], 32 bytes each
        self._block_segment = torch.tensor(block_segment, dtype=torch.int32).to(dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self._lib = _lib.load()
        self._ws_bytes = int(self._lib.zira_optim_tail_workspace_bytes(n))
        if self._ws_bytes != 8 * len(block_segment):
            raise RuntimeError("zira_optim_tail_workspace_bytes(%d) = %d: the library cuts the bucket differently" % (n, self._ws_bytes))
        self._ws = torch.zeros(self._ws_bytes // 8, dtype=torch.float64, device=dev)
        self.norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.amp = bool(amp)
        if self.amp:
            self._amp_ws_bytes = int(self._lib.zira_optim_tail_amp_workspace_bytes(n))
            if self._amp_ws_bytes < self._ws_bytes + 16 + 4 * len(block_segment) or self._amp_ws_bytes % 8:
                raise RuntimeError("zira_optim_tail_amp_workspace_bytes(%d) = %d" % (n, self._amp_ws_bytes))
            self._amp_ws = torch.zeros(self._amp_ws_bytes // 8, dtype=torch.float64, device=dev)
            self._step_dev = torch.zeros((), dtype=torch.int32, device=dev)
            self.found_inf = torch.zeros((), dtype=torch.float32, device=dev)

    def _views(self, flat, i):
        return flat[self.starts[i]:self.starts[i] + self.numels[i]].view_as(self.params[i])

    def step(self, lrs, do_step=True, max_norm=0.1):
        """Norm, clip and -- with ``do_step`` -- AdamW and gradient clear, on the current stream.  ``lrs``: one learning rate
        per group.  ``do_step=False`` (an accumulation iteration) leaves ``grad * scale`` in the bucket and the norm in
        ``norm``; parameters, moments and step counter stay as they are."""
        lrs = [float(x) for x in lrs]
        if len(lrs) < self.n_groups or len(lrs) > MAX_GROUPS:
            raise ValueError("NativeOptimTail.step: %d learning rates for %d groups" % (len(lrs), self.n_groups))
        b1, b2 = self.betas
        bc1 = bc2 = bc2_sqrt = 1.0
        if do_step:
            t = self.step_count + 1
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            bc2_sqrt = math.sqrt(bc2)
        g, n, lib = self.flat_grad, self.flat_grad.numel(), self._lib
        c_lrs = (ctypes.c_double * len(lrs))(*lrs)
        with torch.cuda.device(g.device):
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib.zira_grad_sqnorm_f32(g.data_ptr(), n, self._ws.data_ptr(), self._ws_bytes, stream)
            if rc != 0:
                raise RuntimeError("zira_grad_sqnorm_f32 failed: hipError %d" % rc)
            rc = lib.zira_clip_adamw_f32(g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n,
                                         self._segments.data_ptr(), len(self.params), self._block_segment.data_ptr(), c_lrs,
                                         len(lrs), b1, b2, self.eps, self.weight_decay, bc1, bc2, bc2_sqrt, float(max_norm),
                                         1 if do_step else 0, self.norm.data_ptr(), self._ws.data_ptr(), self._ws_bytes, stream)
            if rc != 0:
                raise RuntimeError("zira_clip_adamw_f32 failed: hipError %d" % rc)
        if do_step:
            self.step_count += 1

    def step_amp(self, lrs, scale, growth_tracker, growth_factor, backoff_factor, growth_interval, max_norm=0.1):
        """The fp16 tail on the current stream, two launches, no host read: the bucket holds gradients of ``scale`` times
        the loss.  ``scale`` (0-dim fp32) and ``growth_tracker`` (0-dim int32) are the ``GradScaler``'s device tensors and
        are updated in place as ``scaler.update()`` would; ``norm`` gets the norm of the unscaled gradients (inf or NaN where
        they are), ``found_inf`` 0.0 or 1.0.  With an inf or a NaN in the bucket parameters, moments and the step counter
        stay as they are; the bucket is cleared either way."""
        if not self.amp:
            raise RuntimeError("NativeOptimTail.step_amp: built without amp=True")
        lrs = [float(x) for x in lrs]
        if len(lrs) < self.n_groups or len(lrs) > MAX_GROUPS:
            raise ValueError("NativeOptimTail.step_amp: %d learning rates for %d groups" % (len(lrs), self.n_groups))
        g = self.flat_grad
        for name, t, dtype in (("scale", scale, torch.float32), ("growth_tracker", growth_tracker, torch.int32)):
            if not (torch.is_tensor(t) and t.device == g.device and t.dtype == dtype and t.numel() == 1):
                raise ValueError("NativeOptimTail.step_amp: %s must be one %s value on %s" % (name, dtype, g.device))
        n, lib = g.numel(), self._lib
        c_lrs = (ctypes.c_double * len(lrs))(*lrs)
        with torch.cuda.device(g.device):
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib.zira_grad_sqnorm_amp_f32(g.data_ptr(), n, scale.data_ptr(), self._step_dev.data_ptr(),
                                              self._amp_ws.data_ptr(), self._amp_ws_bytes, stream)
            if rc != 0:
                raise RuntimeError("zira_grad_sqnorm_amp_f32 failed: hipError %d" % rc)
            rc = lib.zira_clip_adamw_amp_f32(g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n,
                                             self._segments.data_ptr(), len(self.params), self._block_segment.data_ptr(), c_lrs,
                                             len(lrs), self.betas[0], self.betas[1], self.eps, self.weight_decay, float(max_norm),
                                             scale.data_ptr(), growth_tracker.data_ptr(), self._step_dev.data_ptr(),
                                             float(growth_factor), float(backoff_factor), int(growth_interval),
                                             self.norm.data_ptr(), self.found_inf.data_ptr(), self._amp_ws.data_ptr(),
                                             self._amp_ws_bytes, stream)
            if rc != 0:
                raise RuntimeError("zira_clip_adamw_amp_f32 failed: hipError %d" % rc)

    def sync_step_count(self):
        """Read the device step counter of an amp tail into ``step_count`` (one host read) and return it."""
        if self.amp:
            self.step_count = int(self._step_dev.item())
        return self.step_count

    def _check_same_params(self, optimizer):
        theirs = [p for grp in optimizer.param_groups for p in grp["params"]]
        if len(theirs) != len(self.params) or {id(p) for p in theirs} != {id(p) for p in self.params}:
            raise ValueError("NativeOptimTail: the optimizer holds other parameters than this tail")

    def export_to(self, optimizer):
        """Write moments and step count into ``optimizer.state`` (a ``torch.optim.AdamW`` over the same parameters), in the
        form its own first step would have created.  (An amp tail reads its device step counter first.)"""
        self._check_same_params(optimizer)
        self.sync_step_count()
        for grp in optimizer.param_groups:
            on_device = bool(grp.get("fused")) or bool(grp.get("capturable"))
            for p in grp["params"]:
                i = next(k for k, q in enumerate(self.params) if q is p)
                if self.step_count == 0:
                    optimizer.state.pop(p, None)
                    continue
                step = torch.tensor(float(self.step_count), dtype=torch.float32, device=p.device if on_device else "cpu")
                optimizer.state[p] = {"step": step, "exp_avg": self._views(self.exp_avg, i).clone(),
                                      "exp_avg_sq": self._views(self.exp_avg_sq, i).clone()}

    def import_from(self, optimizer):
        """Take moments and step count from ``optimizer.state``; a parameter without state there starts from zero."""
        self._check_same_params(optimizer)
        steps = set()
        for i, p in enumerate(self.params):
            st = optimizer.state.get(p)
            if not st:
                self._views(self.exp_avg, i).zero_()
                self._views(self.exp_avg_sq, i).zero_()
                steps.add(0)
                continue
            if st.get("amsgrad") or "max_exp_avg_sq" in st:
                raise ValueError("NativeOptimTail: amsgrad state is not served")
            self._views(self.exp_avg, i).copy_(st["exp_avg"])
            self._views(self.exp_avg_sq, i).copy_(st["exp_avg_sq"])
            steps.add(int(round(float(st["step"]))))
        if len(steps) != 1:
            raise ValueError("NativeOptimTail: the optimizer's parameters are at different steps: %s" % sorted(steps))
        self.step_count = steps.pop()
        if self.amp:
            self._step_dev.fill_(self.step_count)
