"""Model exponential moving average, the reference's ``groundingdino/util/ema.py`` name for name (``EMAState``,
``EMAUpdater``, ``may_build_model_ema``, ``may_get_ema_checkpointer``, ``get_model_ema_state``, ``apply_model_ema``,
``apply_model_ema_and_restore``; the config arguments are plain keyword arguments, ``EMAHook`` is ``ZiraTrainer(model_ema=)``).

``update_reference`` is the reference's ``EMAUpdater.update`` op for op: the definition, the path of CPU tensors and of
everything the kernel declines.  With ``Switches.native_ema`` the fp32 CUDA tensors -- all but a handful of the model's ~1040
-- are averaged by ONE launch (csrc/ema.hip) instead of two ``_foreach`` passes, ``apply_and_restore`` is two swap launches
instead of a clone of the model, and init / apply are one copy launch.  The averaged values of those tensors live in one flat
fp32 buffer owned by the ``EMAState``; ``state[name]`` is a view into it, so ``state_dict()`` has the reference's keys and
shapes and checkpoints pass between the two.  The model's tensors stay where they are: the kernel reaches them through a
device table of segments (pointer, start in the flat buffer, numel) and a per-block index, the layout of optim_tail.py with
every segment started on a multiple of 4 elements.  The table is rebuilt when the model's tensors or any ``data_ptr`` change
(checked on the host at every call, by count and pointers).

The reference's expression for buffers that are neither fp32 nor fp16 (``ema.copy_(ema * decay + val * (1 - decay))``)
truncates on integer buffers; it is kept as it is."""
import copy
import itertools
import logging
from contextlib import contextmanager
from typing import List

import torch

from . import _lib
from .transformer import Switches

logger = logging.getLogger(__name__)

CHUNK = _lib.CONSTANTS["ZIRA_EMA_CHUNK"]        # elements of the flat index space per block
ALIGN = 4           # every segment starts on a multiple of 4 elements: 16 bytes, the phase of a tensor from the allocator
MAX_N = _lib.CONSTANTS["ZIRA_EMA_MAX_N"]
_lib.assert_int64_rows(_lib.EmaSegment, ("param", "start", "numel"))      # the rows _table_for uploads
# ``torch._foreach_add_(ema, p, alpha=a)`` computes ``ema + a * p``: True where the library's kernel holds that as one fused
# multiply-add, False where it rounds the product first.  tests/test_ema_gpu.py decides it (bit equality with the chain on
# the same device).  Found on an MI355X: contracted (the other form differs in a tenth of the elements); DESIGN.md.
ADD_ALPHA_CONTRACTED = True


def plan_segments(numels, chunk=CHUNK, align=ALIGN):
    """Host-side layout of the flat buffer for tensors of the given sizes: ``(starts, block_segment, n)``.  ``starts[s]`` is
    segment s's offset, the segments in order, each on the next multiple of ``align``; ``n`` is the end of the last one.
    ``block_segment`` as ``block_index`` gives it."""
    numels = [int(x) for x in numels]
    assert len(numels) >= 1 and all(x >= 1 for x in numels), "an empty tensor has no place in the flat buffer"
    starts, off = [], 0
    for x in numels:
        off = (off + align - 1) // align * align
        starts.append(off)
        off += x
    return starts, block_index(starts, numels, off, chunk), off


def block_index(starts, numels, n, chunk=CHUNK):
    """``block_segment[b]``: the first segment that ends behind flat element ``b * chunk`` -- the one holding it or, where it
    lies in a gap, the next one (``len(starts)`` where there is none); the kernel walks on from there while segments start
    inside the block.  (optim_tail.plan_segments' loop, with gaps allowed.)"""
    block_segment, s = [], 0
    for b in range((n + chunk - 1) // chunk):
        while s < len(starts) and starts[s] + numels[s] <= b * chunk:
            s += 1
        block_segment.append(s)
    return block_segment


def _on_device(device, t) -> bool:
    """``t`` lives where ``device`` (a string or torch.device; an index-less "cuda" is any index) says."""
    d = torch.device(device)
    return d.type == t.device.type and (d.index is None or d.index == t.device.index)


class EMAState(object):
    def __init__(self):
        self.state = {}
        self._flat = None        # the flat fp32 buffer the packed entries of ``state`` are views of
        self._layout = {}        # name -> (start, numel) in ``_flat``
        self._table = None       # (key, segments, block_segment, n_segments) of the latest launch

    @classmethod
    def FromModel(cls, model: torch.nn.Module, device: str = ""):
        ret = cls()
        ret.save_from(model, device)
        return ret

    # ---- the flat buffer ---------------------------------------------------------------------------------------------------
    def _allocate(self, shapes, device):
        """A fresh flat buffer for ``shapes`` (name -> torch.Size), zeroed; returns name -> view."""
        names = list(shapes)
        starts, _, n = plan_segments([shapes[k].numel() for k in names])
        if n > MAX_N:
            return {}
        self._flat = torch.zeros(n, dtype=torch.float32, device=device)
        self._layout = {k: (s, shapes[k].numel()) for k, s in zip(names, starts)}
        self._table = None
        return {k: self._flat[s:s + shapes[k].numel()].view(shapes[k]) for k, s in zip(names, starts)}

    def _pack(self):
        """Move every fp32 CUDA entry of ``state`` into one flat buffer (no-op where they are in one already)."""
        self._table = None
        if not Switches.native_ema:
            return
        cand = {k: v for k, v in self.state.items() if v.is_cuda and v.dtype == torch.float32 and v.numel() >= 1}
        if not cand:
            self._flat, self._layout = None, {}
            return
        dev = next(iter(cand.values())).device
        cand = {k: v for k, v in cand.items() if v.device == dev}
        if self._flat is not None and self._flat.device == dev and set(cand) == set(self._layout) and all(
                v.data_ptr() == self._flat.data_ptr() + 4 * self._layout[k][0] for k, v in cand.items()):
            return
        views = self._allocate({k: v.shape for k, v in cand.items()}, dev)
        for k, view in views.items():
            view.copy_(cand[k])
            self.state[k] = view

    def _serves(self, name, val) -> bool:
        """The kernel reaches model tensor ``val`` and its twin: fp32, contiguous, on the flat buffer's device."""
        lay = self._layout.get(name)
        return (lay is not None and val.is_cuda and val.dtype == torch.float32 and val.device == self._flat.device
                and val.is_contiguous() and val.numel() == lay[1] and val.numel() >= 1)

    def _table_for(self, served):
        """Device table and per-block index for ``served`` [(name, model tensor)]; rebuilt only when a start or a pointer moved."""
        key = tuple((self._layout[name][0], val.data_ptr()) for name, val in served)
        if self._table is not None and self._table[0] == key:
            return self._table[1:]
        rows = sorted((start, ptr, self._layout[name][1]) for (start, ptr), (name, _) in zip(key, served))
        starts, numels = [r[0] for r in rows], [r[2] for r in rows]
        dev = self._flat.device
        segments = torch.tensor([[ptr, start, numel] for start, ptr, numel in rows], dtype=torch.int64).to(dev)  # zira_ema_segment[]
        block_segment = torch.tensor(block_index(starts, numels, self._flat.numel()), dtype=torch.int32).to(dev)
        self._table = (key, segments, block_segment, len(rows))
        return self._table[1:]

    def _launch(self, kind, served, decay=0.0, alpha=0.0, to_model=0):
        """One launch of csrc/ema.hip over ``served`` on the current stream."""
        segments, block_segment, n_segments = self._table_for(served)
        lib, flat = _lib.load(), self._flat
        with torch.cuda.device(flat.device):
            stream = torch.cuda.current_stream().cuda_stream
            head = (flat.data_ptr(), flat.numel(), segments.data_ptr(), n_segments, block_segment.data_ptr())
            if kind == "update":
                rc = lib.zira_ema_update_f32(*head, float(decay), float(alpha), 1 if ADD_ALPHA_CONTRACTED else 0, stream)
            elif kind == "swap":
                rc = lib.zira_ema_swap_f32(*head, stream)
            else:
                rc = lib.zira_ema_copy_f32(*head, int(to_model), stream)
        if rc != 0:
            raise RuntimeError("zira_ema_%s_f32 failed: code %d" % (kind, rc))

    def _split(self, model):
        """The model's (name, tensor) pairs as (served by the kernel, the rest), both in the iterator's order."""
        served, rest = [], []
        native = Switches.native_ema and self._flat is not None
        for name, val in self.get_model_state_iterator(model):
            (served if native and self._serves(name, val) else rest).append((name, val))
        return served, rest

    # ---- the reference's surface -------------------------------------------------------------------------------------------
    def save_from(self, model: torch.nn.Module, device: str = ""):
        """Save model state from `model` to this object"""
        items = [(name, val.detach()) for name, val in self.get_model_state_iterator(model)]
        served = []
        if Switches.native_ema:
            served = [(k, v) for k, v in items if v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() >= 1
                      and (not device or _on_device(device, v))]
            served = [(k, v) for k, v in served if v.device == served[0][1].device]
        views = self._allocate({k: v.shape for k, v in served}, served[0][1].device) if served else {}
        if not views:
            self._flat, self._layout, self._table, served = None, {}, None, []
        for name, val in items:
            if name in views:
                self.state[name] = views[name]
            else:
                val = val.clone()
                self.state[name] = val.to(device) if device else val
        if served:
            self._launch("copy", served, to_model=0)

    def apply_to(self, model: torch.nn.Module):
        """Apply state to `model` from this object"""
        with torch.no_grad():
            served, rest = self._split(model)
            for name, val in rest:
                assert (
                    name in self.state
                ), f"Name {name} not existed, available names {self.state.keys()}"
                val.copy_(self.state[name])
            if served:
                self._launch("copy", served, to_model=1)

    def swap_with(self, model: torch.nn.Module):
        """Exchange the model's tensors with their averaged twins: one launch for the packed ones, three copies each for the
        few others.  Twice is the identity."""
        with torch.no_grad():
            served, rest = self._split(model)
            for name, val in rest:
                assert name in self.state, f"Name {name} not existed, available names {self.state.keys()}"
                old = val.detach().clone()
                val.copy_(self.state[name])
                self.state[name].copy_(old)
            if served:
                self._launch("swap", served)

    @contextmanager
    def apply_and_restore(self, model):
        first = next(self.get_model_state_iterator(model), None)
        if Switches.native_ema and self._flat is not None and first is not None and first[1].device == self.device:
            # inside the context this object holds the model's own weights; the swap back restores both, also when the body raises
            self.swap_with(model)
            try:
                yield self
            finally:
                self.swap_with(model)
            return
        old_state = EMAState.FromModel(model, self.device)
        self.apply_to(model)
        yield old_state
        old_state.apply_to(model)

    def get_ema_model(self, model):
        ret = copy.deepcopy(model)
        self.apply_to(ret)
        return ret

    @property
    def device(self):
        if not self.has_inited():
            return None
        return next(iter(self.state.values())).device

    def to(self, device):
        for name in self.state:
            self.state[name] = self.state[name].to(device)
        self._pack()
        return self

    def has_inited(self):
        return self.state

    def clear(self):
        self.state.clear()
        self._flat, self._layout, self._table = None, {}, None
        return self

    def get_model_state_iterator(self, model):
        param_iter = model.named_parameters()
        buffer_iter = model.named_buffers()
        return itertools.chain(param_iter, buffer_iter)

    def state_dict(self):
        return self.state

    def load_state_dict(self, state_dict, strict: bool = True):
        self.clear()
        for x, y in state_dict.items():
            self.state[x] = y
        return torch.nn.modules.module._IncompatibleKeys(
            missing_keys=[], unexpected_keys=[]
        )

    def adopt_missing(self, model):
        """Entries for model tensors this state has none for (prompt-pool entries that ``add_cls_prompt`` created after the
        last update), initialised from the model.  The reference has no such step: its ``apply_to`` asserts on them."""
        missing = [(name, val) for name, val in self.get_model_state_iterator(model) if name not in self.state]
        for name, val in missing:
            self.state[name] = val.detach().clone().to(self.device)
        if missing:
            self._pack()
        return [name for name, _ in missing]

    def __repr__(self):
        ret = f"EMAState(state=[{','.join(self.state.keys())}])"
        return ret


def update_reference(state: EMAState, model, decay: float, device: str = ""):
    """The reference's ``EMAUpdater.update`` (+ ``_ema_avg``), op for op, on whatever device the tensors live."""
    with torch.no_grad():
        ema_param_list = []
        param_list = []
        for name, val in state.get_model_state_iterator(model):
            ema_val = state.state[name]
            if device:
                val = val.to(device)
            if val.dtype in [torch.float32, torch.float16]:
                ema_param_list.append(ema_val)
                param_list.append(val)
            else:
                ema_val.copy_(ema_val * decay + val * (1.0 - decay))
        torch._foreach_mul_(ema_param_list, decay)
        torch._foreach_add_(ema_param_list, param_list, alpha=1 - decay)


class EMAUpdater(object):
    """Model Exponential Moving Average: keeps a moving average of everything in the model state_dict (parameters and
    buffers, frozen ones included), as the reference's class of this name."""

    def __init__(self, state: EMAState, decay: float = 0.999, device: str = ""):
        self.decay = decay
        self.device = device

        self.state = state

    def init_state(self, model):
        self.state.clear()
        self.state.save_from(model, self.device)

    def update(self, model):
        if not Switches.native_ema:
            return update_reference(self.state, model, self.decay, self.device)
        with torch.no_grad():
            served, rest = self.state._split(model)
            if self.device:
                rest = rest + [(k, v) for k, v in served if not _on_device(self.device, v)]
                served = [(k, v) for k, v in served if _on_device(self.device, v)]
            ema_param_list: List[torch.Tensor] = []
            param_list: List[torch.Tensor] = []
            for name, val in rest:      # the reference's own expressions (update_reference) for what the kernel declines
                ema_val = self.state.state[name]
                if self.device:
                    val = val.to(self.device)
                if val.dtype in [torch.float32, torch.float16]:
                    ema_param_list.append(ema_val)
                    param_list.append(val)
                else:
                    ema_val.copy_(ema_val * self.decay + val * (1.0 - self.decay))
            if served:
                self.state._launch("update", served, decay=self.decay, alpha=1 - self.decay)
            if ema_param_list:
                torch._foreach_mul_(ema_param_list, self.decay)
                torch._foreach_add_(ema_param_list, param_list, alpha=1 - self.decay)


def _remove_ddp(model):
    from torch.nn.parallel import DistributedDataParallel

    if isinstance(model, DistributedDataParallel):
        return model.module
    return model


def may_build_model_ema(model, enabled: bool = False):
    if not enabled:
        return
    model = _remove_ddp(model)
    assert not hasattr(
        model, "ema_state"
    ), "Name `ema_state` is reserved for model ema."
    model.ema_state = EMAState()
    logger.info("Using Model EMA.")


def may_get_ema_checkpointer(model, enabled: bool = False):
    if not enabled:
        return {}
    model = _remove_ddp(model)
    return {"ema_state": model.ema_state}


def get_model_ema_state(model):
    """Return the ema state stored in `model`"""
    model = _remove_ddp(model)
    assert hasattr(model, "ema_state")
    ema = model.ema_state
    return ema


def apply_model_ema(model, state=None, save_current=False):
    """Apply ema stored in `model` to model; with ``save_current`` returns the model's previous state."""
    model = _remove_ddp(model)

    if state is None:
        state = get_model_ema_state(model)

    if save_current:
        # save current model state
        old_state = EMAState.FromModel(model, state.device)
    state.apply_to(model)

    if save_current:
        return old_state
    return None


@contextmanager
def apply_model_ema_and_restore(model, state=None):
    """Apply ema stored in `model` to model for the length of the context (``EMAState.apply_and_restore``: two swap launches
    where the state lives on the model's device, the reference's clone and two copies elsewhere)."""
    model = _remove_ddp(model)

    if state is None:
        state = get_model_ema_state(model)

    with state.apply_and_restore(model) as old_state:
        yield old_state
