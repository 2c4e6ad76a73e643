"""Host side of the native training tail (ziragroundingdino_amd/optim_tail.py): the segment planning against a loop over
every flat element, the agreement of the planning with the library's own cut of the bucket, and ``supported()`` declining
CPU tensors so that a CPU trainer keeps the torch path."""
import os

import pytest
import torch
from torch import nn

from ziragroundingdino_amd import optim_tail
from ziragroundingdino_amd.train import ZiraTrainer

NUMELS = [1, 3, 5, 255, 4103, 65536]
GROUPS = [0, 1, 0, 1, 0, 1]


def _owner_of_every_element(numels):
    owner = []
    for s, x in enumerate(numels):
        owner += [s] * x
    return owner


@pytest.mark.parametrize("numels,groups", [(NUMELS, GROUPS), ([4096], [0]), ([4096, 1], [1, 0]), ([4095, 2, 4095, 8192, 7], [0, 0, 1, 2, 7])])
def test_segment_planning_matches_a_loop_over_the_elements(numels, groups):
    chunk = optim_tail.CHUNK
    starts, block_segment = optim_tail.plan_segments(numels, groups)
    owner = _owner_of_every_element(numels)
    n = len(owner)
    # offsets: packed, in order
    assert starts == [owner.index(s) for s in range(len(numels))]
    assert all(owner[starts[s] + numels[s] - 1] == s for s in range(len(numels)))
    # one entry per block of the flat index space, naming the segment of the block's first element
    assert len(block_segment) == (n + chunk - 1) // chunk
    assert block_segment == [owner[b * chunk] for b in range(len(block_segment))]
    # the walk the kernel does from there (while segments start inside the block) reaches every element exactly once,
    # with its own segment's offset and group
    seen = [0] * n
    for b, s in enumerate(block_segment):
        cs, ce = b * chunk, min(n, (b + 1) * chunk)
        while s < len(numels) and starts[s] < ce:
            for i in range(max(starts[s], cs), min(starts[s] + numels[s], ce)):
                assert owner[i] == s and groups[owner[i]] == groups[s] and 0 <= i - starts[s] < numels[s]
                seen[i] += 1
            s += 1
    assert seen == [1] * n


def test_model_of_the_gpu_tests_covers_the_paths():
    """The sizes the GPU tests use: starts on and off the 16-byte grid (0, 1, 4, 9, 264, 4367), single elements, a segment
    that straddles a block boundary and one longer than a block."""
    starts, _ = optim_tail.plan_segments(NUMELS, GROUPS)
    assert starts == [0, 1, 4, 9, 264, 4367] and [s % 4 for s in starts] == [0, 1, 0, 1, 0, 3]
    assert sum(NUMELS) > optim_tail.CHUNK * 16 and NUMELS[-1] > optim_tail.CHUNK      # many blocks, a segment longer than one
    assert any(s // optim_tail.CHUNK != (s + x - 1) // optim_tail.CHUNK for s, x in zip(starts, NUMELS))   # a straddling one


def test_planning_agrees_with_the_library():
    """The constants the Python side plans with are the header's: the library answers one double of workspace per block."""
    from ziragroundingdino_amd import _lib

    lib = _lib.load()
    for n in (1, 4095, 4096, 4097, sum(NUMELS), optim_tail.MAX_N):
        _, block_segment = optim_tail.plan_segments([n], [0])
        assert lib.zira_optim_tail_workspace_bytes(n) == 8 * len(block_segment)
    assert lib.zira_optim_tail_workspace_bytes(0) == 0 and lib.zira_optim_tail_workspace_bytes(optim_tail.MAX_N + 1) == 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(optim_tail.__file__)))
    with open(os.path.join(root, "include", "zira_msda.h")) as f:
        header = f.read()
    assert "#define ZIRA_OPTIM_TAIL_CHUNK %d\n" % optim_tail.CHUNK in header
    assert "#define ZIRA_OPTIM_TAIL_MAX_GROUPS %d\n" % optim_tail.MAX_GROUPS in header


def test_supported_declines_cpu_tensors_and_foreign_gradients():
    ps = [nn.Parameter(torch.randn(x)) for x in (3, 5)]
    flat = torch.zeros(8)
    off = 0
    for p in ps:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    assert optim_tail.supported(ps, flat) is False
    assert optim_tail.supported([], flat) is False
    with pytest.raises(RuntimeError, match="not served"):
        optim_tail.NativeOptimTail(ps, flat, [0, 1])


def test_a_cpu_trainer_keeps_the_torch_path(monkeypatch):
    class _M(nn.Module):
        def __init__(self):
            super().__init__()
            self.adapter = nn.Linear(4, 4)

        def before_train(self):
            pass

    monkeypatch.setattr(ZiraTrainer, "native_tail", True)
    trainer = ZiraTrainer(_M(), tuned_gemms=False)
    assert trainer._tail is None and trainer.last_grad_norm is None
    trainer.export_tail_state()     # (nothing to carry: no-ops)
    trainer.import_tail_state()
