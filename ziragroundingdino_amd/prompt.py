"""The substitution of the prompt-tuning baseline (``use_prompt_tuning``): the rows of the encoded text that belong to a
category with an entry in ``prompt_memory_pool`` are replaced by that entry, a trained ``[n_tok, hidden_dim]`` tensor under the
key ``-name-`` (reference models/GroundingDINO/groundingdino_dt.py: ``add_cls_prompt`` :379-437 makes the entries, ``forward``
:521-531 substitutes them, in training and in eval).  The dual-branch class this package mirrors carries the switch and drops
its use; the piece is taken from the sibling, as the gated adapter and the trained class head were.

The reference walks images x categories and writes through a boolean mask each time: a ``nonzero`` with a host read and
several launches per pair, and the same again backward.  Here the masks are read ONCE per (captions, pool), by
``build_table``, into two index tables; after that

* ``substitute`` is one autograd node over csrc/prompt.hip (C ABI in include/zira_prompt.h): one launch forward, one launch
  backward, no host read, no atomics, capturable.  It serves fp32 CUDA tensors outside autocast inside the header's limits,
  under ``transformer.Switches.native_prompt``.  The pool entries stay the separate parameters they are (a device table of
  segment pointers, the layout of optim_tail.py / ema.py); their gradients are row ranges of one ``[R, D]`` buffer, which
  autograd then accumulates into each leaf's ``.grad`` as it does for any node: one launch per entry named in the captions.
* ``substitute_reference`` is the definition in torch ops: from the masks it is the loop itself, from a table it is one
  indexed write.  It serves CPU tensors, other dtypes, autocast, shapes the header declines and ``FORCE_REFERENCE``.

The text-memory replay (``use_prompt_memory``) reads the same tables: ``memory_loss`` is the reference's ``loss_prompt_memory``
(:509-519, ``replay_memory`` :824-834), ``L1Loss(mean)`` between the encoded text and its copy with the learned categories' rows
replaced by their stored entries -- one autograd node over csrc/prompt_memory.hip (C ABI in include/zira_prompt_memory.h) that
returns the scalar, under ``transformer.Switches.native_prompt_memory``; ``memory_loss_reference`` is its definition in torch ops.
"""
from typing import Mapping, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .dense import _zeroed_once

FORCE_REFERENCE = False      # True: every call is substitute_reference
MAX_B, MAX_T, MAX_D = (_lib.PROMPT_CONSTANTS[k] for k in ("ZIRA_PROMPT_MAX_B", "ZIRA_PROMPT_MAX_T", "ZIRA_PROMPT_MAX_D"))
MAX_SEGMENTS, MAX_ROWS = _lib.PROMPT_CONSTANTS["ZIRA_PROMPT_MAX_SEGMENTS"], _lib.PROMPT_CONSTANTS["ZIRA_PROMPT_MAX_ROWS"]
_lib.assert_int64_rows(_lib.PromptSegment, ("param", "rows"))      # the rows PromptTable.segments uploads


def pool_key(name: str) -> str:
    """The reference's key of a class's pool entry."""
    return "-{}-".format(name)


class PromptTable:
    """What ``build_table`` returns.  Host side: ``keys`` / ``rows`` of the pool segments, ``seg_row`` [B, T, 2] int32 --
    (segment, row) per token or (-1, -1) --, ``occ_start`` [R + 1] and ``occ`` int32, the positions ``b * T + t`` of every pool
    row, ascending (R = ``n_rows``, the pool's rows numbered segment after segment).  ``on(device)`` holds the uploads."""

    def __init__(self, keys, rows, seg_row, occ_start, occ):
        self.keys, self.rows = list(keys), [int(r) for r in rows]
        self.seg_row, self.occ_start, self.occ = seg_row, occ_start, occ
        self.B, self.T = int(seg_row.shape[0]), int(seg_row.shape[1])
        self.n_rows, self.n_occ = int(sum(self.rows)), int(occ.numel())
        self.row_start = [0]
        for r in self.rows:
            self.row_start.append(self.row_start[-1] + r)
        self._device, self._segments, self._workspace = {}, {}, {}

    def on(self, device):
        """(table int32 [B, T, 2], occ_start, occ (at least one element), and for the op chain the int64 index vectors
        b, t, pool row of every substituted position) on ``device``, uploaded once."""
        device = torch.device(device)
        held = self._device.get(device)
        if held is None:
            flat = self.seg_row.reshape(-1, 2)
            pos = torch.nonzero(flat[:, 0] >= 0).reshape(-1)
            start = torch.tensor(self.row_start, dtype=torch.int64)
            pool_row = start[flat[pos, 0].long()] + flat[pos, 1].long()
            occ = self.occ if self.n_occ else torch.zeros(1, dtype=torch.int32)
            held = self._device[device] = tuple(t.to(device) for t in (
                self.seg_row.contiguous(), self.occ_start, occ, pos // self.T, pos % self.T, pool_row))
        return held

    def segments(self, params):
        """The device table of segment pointers (zira_prompt_segment[]) for ``params``; uploaded again only when a pointer moved
        (checked on the host, by value)."""
        dev = params[0].device
        key = tuple(p.data_ptr() for p in params)
        held = self._segments.get(dev)
        if held is None or held[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("prompt.substitute: a pool entry moved; run once outside the capture first")
            held = self._segments[dev] = (key, torch.tensor([[ptr, r] for ptr, r in zip(key, self.rows)], dtype=torch.int64).to(dev))
        return held[1]

    def workspace(self, device, nbytes):
        """``memory_loss``'s forward workspace (ticket word + the blocks' doubles) on ``device``: allocated ZEROED once, outside
        any capture -- the kernel leaves the ticket at zero again, so neither a later call nor a graph replay clears it.  One
        workspace serves one stream at a time: an eager call on another stream than the last one first waits for that stream."""
        return _zeroed_once(self._workspace, torch.device(device), nbytes, torch.uint8, 0,
                            "prompt.memory_loss: the table has no workspace on %s")


def build_table(names_list, cate_to_token_mask_list, pool_keys: Sequence[str], pool_rows: Sequence[int], T: int) -> PromptTable:
    """The substitution of one batch of captions as index tables.  ``names_list[b][c]`` names category c of image b,
    ``cate_to_token_mask_list[b]`` is its [n_cat, width] boolean token mask, ``pool_keys`` / ``pool_rows`` are the keys
    (``-name-``) and row counts of the pool entries (the segments, in this order), ``T`` the token count of the encoded text.
    The i-th set token of a category's mask takes row i of the category's entry.  Where two categories of an image claim one
    token the later one holds it, as the reference's loop order gives.  The masks are read to the host here, once.

    Raises ``ValueError`` where a category's token count differs from its entry's row count (the reference fails with a shape
    error there) and where a mask is wider than the encoded text (an index error there)."""
    index = {k: s for s, k in enumerate(pool_keys)}
    if len(index) != len(pool_keys) or len(pool_keys) != len(pool_rows):
        raise ValueError("build_table: pool keys must be distinct and come with one row count each")
    B = len(cate_to_token_mask_list)
    if len(names_list) != B:
        raise ValueError("build_table: %d name lists for %d mask tensors" % (len(names_list), B))
    seg_row = torch.full((B, int(T), 2), -1, dtype=torch.int32)
    for b, (names, masks) in enumerate(zip(names_list, cate_to_token_mask_list)):
        masks = masks.detach().to("cpu", torch.bool)
        if masks.dim() != 2:
            raise ValueError("build_table: image %d's token masks are not [n_cat, width]" % b)
        if masks.shape[0] and masks.shape[1] > T:
            raise ValueError("build_table: image %d's token masks are %d wide, the encoded text has %d tokens"
                             % (b, masks.shape[1], T))
        # (a caption shorter than the batch's longest gets one empty mask more than it has names, for the [SEP] in front of its
        # padding; the reference's loop fails on it with an IndexError, here an EMPTY surplus mask is passed over)
        if masks.shape[0] > len(names) and bool(masks[len(names):].any()):
            raise ValueError("build_table: image %d has %d token masks and %d names" % (b, masks.shape[0], len(names)))
        for c in range(min(masks.shape[0], len(names))):
            s = index.get(pool_key(names[c]))
            if s is None:
                continue
            tokens = torch.nonzero(masks[c]).reshape(-1)
            if tokens.numel() != int(pool_rows[s]):
                raise ValueError("build_table: class %r has %d tokens in image %d's caption, its pool entry %d rows"
                                 % (names[c], tokens.numel(), b, int(pool_rows[s])))
            seg_row[b, tokens, 0] = s
            seg_row[b, tokens, 1] = torch.arange(tokens.numel(), dtype=torch.int32)
    # the occurrence lists: positions in ascending order (so ascending b), stably grouped by pool row
    row_start = torch.zeros(len(pool_rows) + 1, dtype=torch.int64)
    row_start[1:] = torch.cumsum(torch.tensor([int(r) for r in pool_rows], dtype=torch.int64), 0)
    flat = seg_row.reshape(-1, 2)
    pos = torch.nonzero(flat[:, 0] >= 0).reshape(-1)
    pool_row = row_start[flat[pos, 0].long()] + flat[pos, 1].long()
    order = torch.sort(pool_row, stable=True).indices
    occ = pos[order].to(torch.int32)
    occ_start = torch.zeros(int(row_start[-1]) + 1, dtype=torch.int32)
    occ_start[1:] = torch.cumsum(torch.bincount(pool_row, minlength=int(row_start[-1])), 0).to(torch.int32)
    return PromptTable(pool_keys, pool_rows, seg_row, occ_start, occ)


def _pool_list(keys, pool_params):
    if isinstance(pool_params, (Mapping, torch.nn.ParameterDict)):
        return [pool_params[k] for k in keys]
    return list(pool_params)


def substitute_reference(encoded_text, table_or_masks, pool_params):
    """The definition.  ``table_or_masks`` is ``(names_list, cate_to_token_mask_list)`` -- then this is the loop itself, image by
    image and category by category, one boolean-mask write each, with ``pool_params`` a mapping from ``-name-`` keys -- or a
    ``PromptTable``: the same result as one indexed write (``pool_params`` the mapping, or the entries in the table's order).
    Returns a new tensor; gradients reach ``encoded_text`` outside the substituted rows and the pool entries inside them."""
    out = encoded_text.clone()
    if not isinstance(table_or_masks, PromptTable):
        names_list, masks_list = table_or_masks
        for b, masks in enumerate(masks_list):
            for c in range(len(masks)):
                key = pool_key(names_list[b][c])
                if key in pool_params:
                    out[b, :masks.shape[1], :][masks[c]] = pool_params[key].to(out.dtype)
        return out
    table = table_or_masks
    if table.n_occ == 0:
        return out
    if tuple(encoded_text.shape[:2]) != (table.B, table.T):
        raise ValueError("substitute: a table for [%d, %d] tokens, text of shape %s" % (table.B, table.T, tuple(encoded_text.shape)))
    _, _, _, bi, ti, pool_row = table.on(encoded_text.device)
    rows = torch.cat([p.reshape(-1, encoded_text.shape[-1]) for p in _pool_list(table.keys, pool_params)], 0)
    out[bi, ti] = rows[pool_row].to(out.dtype)
    return out


def native_supported(encoded_text, table: PromptTable, params) -> bool:
    """Shapes, dtypes and placement the kernels take (the switches are the caller's)."""
    x = encoded_text
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and not torch.is_autocast_enabled("cuda") and x.numel() > 0):
        return False
    B, T, D = x.shape
    if (B, T) != (table.B, table.T) or len(params) != len(table.keys) or not params:
        return False
    if not _lib.load().zira_prompt_supported(B, T, D, len(params), table.n_rows):
        return False
    return all(p.dtype == torch.float32 and p.device == x.device and p.is_contiguous() and p.data_ptr() % 16 == 0
               and tuple(p.shape) == (r, D) for p, r in zip(params, table.rows))


def _check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (name, rc))


class _SubstituteNative(Function):
    """(x [B, T, D], table, *pool entries) -> out [B, T, D] through zira_prompt_substitute_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, x, table, *params):
        lib = _lib.load()
        x = x.contiguous()
        B, T, D = x.shape
        dev = x.device
        seg_row, _, _, _, _, _ = table.on(dev)
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _check(lib.zira_prompt_substitute_fwd_f32(x.data_ptr(), seg_row.data_ptr(), table.segments(params).data_ptr(), B, T, D,
                                                      len(params), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "zira_prompt_substitute_fwd_f32")
        ctx.table, ctx.shape, ctx.need_gx = table, (B, T, D), ctx.needs_input_grad[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        table, (B, T, D) = ctx.table, ctx.shape
        g = grad_out.contiguous()
        dev = g.device
        seg_row, occ_start, occ, _, _, _ = table.on(dev)
        g_pool = torch.empty((table.n_rows, D), dtype=torch.float32, device=dev)
        gx = torch.empty_like(g) if ctx.need_gx else None
        with torch.cuda.device(dev):
            _check(lib.zira_prompt_substitute_bwd_f32(g.data_ptr(), seg_row.data_ptr(), occ_start.data_ptr(), occ.data_ptr(), B, T, D,
                                                      table.n_rows, table.n_occ, g_pool.data_ptr(),
                                                      gx.data_ptr() if gx is not None else None,
                                                      torch.cuda.current_stream(dev).cuda_stream),
                   "zira_prompt_substitute_bwd_f32")
        starts = table.row_start
        grads = tuple(g_pool[starts[s]:starts[s + 1]] if ctx.needs_input_grad[2 + s] else None for s in range(len(table.keys)))
        return (gx, None) + grads


def substitute(encoded_text, table: PromptTable, pool_params):
    """``encoded_text`` [B, T, D] with the rows ``table`` names replaced by their pool entries: one autograd node over the HIP
    kernels where they serve, ``substitute_reference`` elsewhere."""
    from .transformer import Switches

    params = _pool_list(table.keys, pool_params)
    if Switches.native_prompt and not FORCE_REFERENCE and native_supported(encoded_text, table, params):
        return _SubstituteNative.apply(encoded_text, table, *params)
    return substitute_reference(encoded_text, table, params)


# ---- the text-memory replay's loss ------------------------------------------------------------------------------------------------

def memory_loss_reference(encoded_text, table_or_masks, pool_params):
    """The definition of ``loss_prompt_memory``: ``L1Loss(mean)(target, encoded_text)``, where ``target`` is ``encoded_text.clone()``
    with the rows of every category that has an entry in ``pool_params`` overwritten by the entry.  ``table_or_masks`` is
    ``(names_list, cate_to_token_mask_list)`` -- then this is the reference's loop itself, image by image and category by category,
    one boolean-mask write each, with ``pool_params`` a mapping from ``-name-`` keys (the caller hands in the learned classes'
    entries); an empty surplus mask behind a caption's names is passed over, as ``build_table`` passes it -- or a ``PromptTable``:
    the same target as one indexed write.  Gradients reach ``encoded_text`` and the entries that require them."""
    if isinstance(table_or_masks, PromptTable):
        target = substitute_reference(encoded_text, table_or_masks, pool_params)
    else:
        names_list, masks_list = table_or_masks
        target = encoded_text.clone()
        for b, masks in enumerate(masks_list):
            for c in range(min(len(masks), len(names_list[b]))):
                key = pool_key(names_list[b][c])
                if key in pool_params:
                    target[b, :masks.shape[1], :][masks[c]] = pool_params[key].to(target.dtype)
    return torch.nn.functional.l1_loss(target, encoded_text)


class _MemoryLossNative(Function):
    """(x [B, T, D], table, *pool entries) -> the scalar loss through zira_pmem_loss_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, x, table, *params):
        lib = _lib.load()
        x = x.contiguous()
        B, T, D = x.shape
        dev = x.device
        seg_row = table.on(dev)[0]
        segments = table.segments(params)
        ws = table.workspace(dev, lib.zira_pmem_workspace_bytes(B, T))
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(lib.zira_pmem_loss_fwd_f32(x.data_ptr(), seg_row.data_ptr(), segments.data_ptr(), B, T, D, len(params),
                                              loss.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "zira_pmem_loss_fwd_f32")
        ctx.save_for_backward(x, *params)
        ctx.table = table
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        lib = _lib.load()
        table = ctx.table
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        B, T, D = x.shape
        dev = x.device
        g = grad_loss.contiguous().to(torch.float32)
        seg_row, occ_start, occ, _, _, _ = table.on(dev)
        need_pool = any(ctx.needs_input_grad[2:])
        g_pool = torch.empty((table.n_rows, D), dtype=torch.float32, device=dev) if need_pool else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            _check(lib.zira_pmem_loss_bwd_f32(g.data_ptr(), x.data_ptr(), seg_row.data_ptr(), table.segments(params).data_ptr(),
                                              occ_start.data_ptr(), occ.data_ptr(), B, T, D, len(params), table.n_rows, table.n_occ,
                                              g_pool.data_ptr() if need_pool else None, gx.data_ptr() if gx is not None else None,
                                              torch.cuda.current_stream(dev).cuda_stream),
                   "zira_pmem_loss_bwd_f32")
        starts = table.row_start
        grads = tuple(g_pool[starts[s]:starts[s + 1]] if ctx.needs_input_grad[2 + s] else None for s in range(len(table.keys)))
        return (gx, None) + grads


def memory_loss(encoded_text, table: PromptTable, pool_params):
    """``loss_prompt_memory`` of ``encoded_text`` [B, T, D] against the pool entries ``table`` names: one autograd node over the HIP
    kernels where they serve (fp32 CUDA tensors outside autocast, inside the header's limits), ``memory_loss_reference``
    elsewhere."""
    from .transformer import Switches

    params = _pool_list(table.keys, pool_params)
    if Switches.native_prompt_memory and not FORCE_REFERENCE and native_supported(encoded_text, table, params):
        return _MemoryLossNative.apply(encoded_text, table, *params)
    return memory_loss_reference(encoded_text, table, params)
