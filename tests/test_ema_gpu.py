"""The model EMA on the GPU (csrc/ema.hip through ziragroundingdino_amd/ema.py): update, swap and copy as one launch each.

The model is the fixture's tiny module (tests/golden/gen_ema_golden.py: fp32 tensors of 1, 3, 4095, 1, 4097, 4096, 17 x 5 and
8192 + 7 elements, an fp16, an int64 and a bool buffer) with every parameter re-pointed at an offset view of a larger
sentinel-filled tensor of its own: the offsets leave the pointers 16-byte aligned or off by 4, 8 and 12 bytes in turn, so runs
whose two addresses share their phase (16-byte accesses with per-lane ends) and runs that do not (per-lane throughout) both
occur, segments start inside blocks, and two tensors are longer than a block.

Bars: bit equality with ``update_reference`` (torch's ``_foreach_mul_`` / ``_foreach_add_(alpha=)`` chain) on the same device;
against the reference's CPU result the derived bound |device - golden| <= 2 k 2^-23 max(|ema|, |p|) after k steps (the device
may round each of the two operations of a step differently from the CPU)."""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from gen_ema_golden import DECAY, SIZES, STEPS, model_state, set_step, tiny_module  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARDS = (4, 1, 2, 3)       # elements in front of parameter i's view: i % 4 -> 0, 4, 8, 12 bytes off the 16-byte grid
PARAMS = ["p%02d" % i for i in range(len(SIZES))]


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "ema_zira_slice.pt"), weights_only=False)


@pytest.fixture
def switches():
    from ziragroundingdino_amd.transformer import Switches

    saved = Switches.native_ema
    yield Switches
    Switches.native_ema = saved


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(view), b.contiguous().view(view))
    return torch.equal(a, b)


class Guarded:
    """The tiny module on the GPU, every parameter a view ``buf[gd:gd + n]`` of its own sentinel-filled allocation."""

    def __init__(self, model=None):
        self.model = (model or tiny_module()).cuda()
        self.bufs = []
        for i, name in enumerate(PARAMS):
            p, gd = getattr(self.model, name), GUARDS[i % 4]
            buf = torch.full((gd + p.numel() + 4,), SENTINEL, device="cuda")
            buf[gd:gd + p.numel()] = p.detach()
            p.data = buf[gd:gd + p.numel()]
            assert p.data_ptr() % 16 == (4 * gd) % 16
            self.bufs.append((buf, gd, p.numel()))

    def guards_untouched(self):
        return all(bool((buf[:gd] == SENTINEL).all()) and bool((buf[gd + n:] == SENTINEL).all()) for buf, gd, n in self.bufs)


def native_state(g, decay=DECAY):
    """A packed state initialised from the model (the copy launch), with its updater."""
    from ziragroundingdino_amd import ema

    state = ema.EMAState()
    updater = ema.EMAUpdater(state, decay=decay, device="")
    updater.init_state(g.model)
    assert state._flat is not None and set(state._layout) == set(PARAMS), "every fp32 tensor is packed"
    return state, updater


def reference_state(g, switches):
    """A state of separate tensors, as the reference keeps it."""
    from ziragroundingdino_amd import ema

    saved, switches.native_ema = switches.native_ema, False
    try:
        state = ema.EMAState.FromModel(g.model)
    finally:
        switches.native_ema = saved
    assert state._flat is None
    return state


def gaps_are_zero(state):
    """Elements of the flat buffer between segments: never written."""
    owned = torch.zeros(state._flat.numel(), dtype=torch.bool, device="cuda")
    for start, numel in state._layout.values():
        owned[start:start + numel] = True
    return bool((state._flat[~owned] == 0).all()) and int((~owned).sum()) > 0


def test_layout_of_the_test_model_covers_the_paths():
    from ziragroundingdino_amd import ema

    g = Guarded()
    state, _ = native_state(g)
    starts = [state._layout[k][0] for k in PARAMS]
    assert all(s % 4 == 0 for s in starts) and state._flat.data_ptr() % 16 == 0
    phases = {(getattr(g.model, k).data_ptr() // 4) % 4 for k in PARAMS}
    assert phases == {0, 1, 2, 3}                               # aligned and off by 4, 8 and 12 bytes
    assert state._flat.numel() > 5 * ema.CHUNK                  # several blocks
    assert any(s // ema.CHUNK != (s + n - 1) // ema.CHUNK for s, n in zip(starts, SIZES))     # a segment across a block boundary
    assert sum(1 for s in starts if s // ema.CHUNK == starts[6] // ema.CHUNK) >= 17            # many segments start in one block
    # init was the copy launch, model -> average: the bits of the model, nothing else touched
    for k, v in model_state(g.model).items():
        assert same_bits(state.state[k], v), k
    assert g.guards_untouched() and gaps_are_zero(state)


@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_update_is_bit_identical_to_the_op_chain_on_the_device(decay, switches):
    """8 steps, after every one: the kernel's state against ``update_reference`` on the same device, int32 views equal.  (Fails
    where ``ADD_ALPHA_CONTRACTED`` is wrong for the library's ``_foreach_add_(alpha=)`` kernel.)"""
    from ziragroundingdino_amd import ema

    g = Guarded()
    state, updater = native_state(g, decay)
    want = reference_state(g, switches)
    for k in range(1, STEPS + 1):
        set_step(g.model, k)
        updater.update(g.model)
        ema.update_reference(want, g.model, decay)
        assert list(state.state) == list(want.state)
        for name in want.state:
            a, b = state.state[name], want.state[name]
            if name in PARAMS:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, name, float((a - b).abs().max()))
            else:
                assert same_bits(a, b), (k, name)
    assert state._table is not None and state._table[3] == len(PARAMS), "one launch over every fp32 tensor"
    assert g.guards_untouched() and gaps_are_zero(state)


def test_the_contraction_setting_is_decided_by_the_data(switches, monkeypatch):
    """The recorded steps cannot tell the two forms of ``ema + alpha * p`` apart (their parameters carry few mantissa bits, and
    with decay 0.5 the product is exact).  Full-mantissa values and decay 0.9 can: the form ``ADD_ALPHA_CONTRACTED`` names
    equals the op chain on this device bit for bit, and the other form does not."""
    from ziragroundingdino_amd import ema

    gen = torch.Generator().manual_seed(5)

    def run(contracted):
        monkeypatch.setattr(ema, "ADD_ALPHA_CONTRACTED", contracted)
        g = Guarded()
        gen.manual_seed(5)
        with torch.no_grad():
            for name in PARAMS:
                getattr(g.model, name).copy_(torch.randn(getattr(g.model, name).shape, generator=gen))
        state, updater = native_state(g, 0.9)
        want = reference_state(g, switches)
        differing = 0
        for _ in range(2):
            with torch.no_grad():
                for name in PARAMS:
                    getattr(g.model, name).copy_(torch.randn(getattr(g.model, name).shape, generator=gen))
            updater.update(g.model)
            ema.update_reference(want, g.model, 0.9)
            differing += sum(int((state.state[k].view(torch.int32) != want.state[k].view(torch.int32)).sum()) for k in PARAMS)
        assert g.guards_untouched()
        return differing

    configured = ema.ADD_ALPHA_CONTRACTED
    right, wrong = run(configured), run(not configured)
    print("elements differing from the op chain over 2 steps: configured form (contracted=%s) %d, the other form %d"
          % (configured, right, wrong))
    assert right == 0 and wrong > 100


def test_update_against_the_references_cpu_result(golden):
    """After k <= 8 steps |device - golden| <= 2 k 2^-23 max(|ema|, |p|) elementwise: two operations per step, each at most one
    rounding (2^-24 relative) away from the CPU's -- doubled for the error carried through ``* decay``."""
    g = Guarded()
    state, updater = native_state(g)
    worst = 0.0
    for k in range(1, STEPS + 1):
        set_step(g.model, k)
        updater.update(g.model)
        for name in PARAMS:
            got, ref = state.state[name].cpu().double(), golden["steps"][k - 1][name].double()
            p = getattr(g.model, name).detach().cpu().double()
            bound = 2 * k * 2.0 ** -23 * torch.maximum(ref.abs(), p.abs())
            err = (got - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (k, name, float(err.max()))
    print("largest |device - golden| / bound over 8 steps: %.3f" % worst)
    for name in ("count", "flag"):      # (single correctly rounded fp32 operations and a truncation: the CPU's bits)
        assert same_bits(state.state[name].cpu(), golden["steps"][-1][name]), name


def test_swap_and_back():
    g = Guarded()
    state, updater = native_state(g)
    set_step(g.model, 1)
    updater.update(g.model)
    model0, state0 = model_state(g.model), {k: v.clone() for k, v in state.state.items()}
    assert not same_bits(model0["p02"], state0["p02"])
    state.swap_with(g.model)
    for k in model0:
        assert same_bits(getattr(g.model, k).detach(), state0[k]), k      # the model holds the old average
        assert same_bits(state.state[k], model0[k]), k                    # the state holds the old model
    assert g.guards_untouched() and gaps_are_zero(state)
    state.swap_with(g.model)
    for k in model0:
        assert same_bits(getattr(g.model, k).detach(), model0[k]) and same_bits(state.state[k], state0[k]), k
    assert g.guards_untouched() and gaps_are_zero(state)
    # the context manager is the two swaps
    with state.apply_and_restore(g.model) as held:
        assert held is state
        assert all(same_bits(getattr(g.model, k).detach(), state0[k]) for k in model0)
    assert all(same_bits(getattr(g.model, k).detach(), model0[k]) and same_bits(state.state[k], state0[k]) for k in model0)


def test_copy_both_directions():
    g = Guarded()
    state, updater = native_state(g)          # (model -> average: checked in the layout test)
    set_step(g.model, 1)
    set_step(g.model, 2)
    kept = {k: v.clone() for k, v in state.state.items()}
    state.apply_to(g.model)                   # average -> model
    for k in kept:
        assert same_bits(getattr(g.model, k).detach(), kept[k]) and same_bits(state.state[k], kept[k]), k
    assert g.guards_untouched() and gaps_are_zero(state)
    set_step(g.model, 3)
    now = model_state(g.model)
    state.save_from(g.model)                  # model -> average again, into a fresh flat buffer
    for k in now:
        assert same_bits(state.state[k], now[k]) and same_bits(getattr(g.model, k).detach(), now[k]), k
    assert g.guards_untouched() and gaps_are_zero(state)


def test_a_moved_parameter_rebuilds_the_table(switches):
    """A parameter whose storage was replaced (``load_state_dict`` copies in place, ``.to()`` and the re-parameterisation do
    not): the next update reads the new tensor."""
    from ziragroundingdino_amd import ema

    g = Guarded()
    state, updater = native_state(g, 0.5)
    want = reference_state(g, switches)
    set_step(g.model, 1)
    updater.update(g.model)
    ema.update_reference(want, g.model, 0.5)
    table = state._table
    updater.update(g.model)
    ema.update_reference(want, g.model, 0.5)
    assert state._table is table, "same tensors: the table is kept"
    g.model.p04.data = g.model.p04.detach().clone() * 3.0
    updater.update(g.model)
    ema.update_reference(want, g.model, 0.5)
    assert state._table is not table
    for name in want.state:
        assert same_bits(state.state[name], want.state[name]), name


def test_update_replays_from_a_graph():
    """Captured once (a plain linear graph), replayed 3 times over parameters changed in place: 3 eager updates."""
    g = Guarded()
    state_a, upd_a = native_state(g)
    state_b, upd_b = native_state(g)
    set_step(g.model, 1)
    upd_a.update(g.model)       # (builds the table outside the capture)
    upd_b.update(g.model)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        upd_a.update(g.model)
    for k in (2, 3, 4):
        set_step(g.model, k)
        graph.replay()
        upd_b.update(g.model)
    torch.cuda.synchronize()
    for name in state_b.state:
        assert same_bits(state_a.state[name], state_b.state[name]), name
    assert not same_bits(state_a.state["p02"], getattr(g.model, "p02").detach())
    assert g.guards_untouched()


def test_declined_inputs_take_the_reference_path(switches):
    from ziragroundingdino_amd import _lib, ema

    # a CPU model
    cpu = tiny_module()
    state = ema.EMAState()
    updater = ema.EMAUpdater(state, decay=0.5)
    updater.init_state(cpu)
    want = ema.EMAState.FromModel(cpu)
    set_step(cpu, 1)
    updater.update(cpu)
    ema.update_reference(want, cpu, 0.5)
    assert state._flat is None and all(same_bits(state.state[k], want.state[k]) for k in want.state)

    # an fp64 parameter and an fp16 buffer beside fp32 tensors on the GPU
    class Mixed(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.linspace(-1, 1, 37))
            self.d = torch.nn.Parameter(torch.linspace(-1, 1, 11, dtype=torch.float64))
            self.register_buffer("h", torch.linspace(-2, 2, 9).half())

    m = Mixed().cuda()
    state = ema.EMAState()
    updater = ema.EMAUpdater(state, decay=0.999)
    updater.init_state(m)
    want = reference_state(type("G", (), {"model": m})(), switches)
    for _ in range(3):
        with torch.no_grad():
            for t in (m.w, m.d, m.h):
                t.mul_(1.25).add_(0.125)
        updater.update(m)
        ema.update_reference(want, m, 0.999)
    assert set(state._layout) == {"w"} and state.state["d"].dtype == torch.float64
    assert all(same_bits(state.state[k], want.state[k]) for k in ("w", "d", "h"))
    with state.apply_and_restore(m):            # the swap takes the other tensors along
        assert all(same_bits(getattr(m, k).detach(), want.state[k]) for k in ("w", "d", "h"))

    # n = 0: the "not served" code, nothing is launched
    lib = _lib.load()
    flat, seg, blk = state._flat, state._table[1], state._table[2]
    assert lib.zira_ema_update_f32(flat.data_ptr(), 0, seg.data_ptr(), 1, blk.data_ptr(), 0.9, 0.1, 1, None) == 1
    assert lib.zira_ema_swap_f32(flat.data_ptr(), 0, seg.data_ptr(), 1, blk.data_ptr(), None) == 1
    assert lib.zira_ema_copy_f32(flat.data_ptr(), 0, seg.data_ptr(), 1, blk.data_ptr(), 1, None) == 1
    torch.cuda.synchronize()
    assert all(same_bits(state.state[k], want.state[k]) for k in ("w", "d", "h"))


def test_trainer_with_the_switch_on_and_off(switches):
    """Two run_steps of the tiny model with ``model_ema`` set, ``native_ema`` on and off: the averaged states are equal bit for
    bit, and the trained parameters are those of a run with ``model_ema=None``."""
    from test_ema_cpu import Trainable
    from ziragroundingdino_amd.train import ZiraTrainer

    def run(native, model_ema):
        switches.native_ema = native
        model = Trainable().cuda().train()
        trainer = ZiraTrainer(model, lr=1e-2, tuned_gemms=False, model_ema=model_ema)
        for it in range(2):
            trainer.run_step(1.0 + it)
        return model

    on, off, none = run(True, dict(decay=0.999)), run(False, dict(decay=0.999)), run(True, None)
    assert on.ema_state._flat is not None and on.ema_state._table[3] == len(PARAMS)
    assert off.ema_state._flat is None and not hasattr(none, "ema_state")
    assert list(on.ema_state.state) == list(off.ema_state.state)
    for k in on.ema_state.state:
        assert same_bits(on.ema_state.state[k], off.ema_state.state[k]), k
    for (k, p), (_, q), (_, r) in zip(on.named_parameters(), off.named_parameters(), none.named_parameters()):
        assert same_bits(p.detach(), r.detach()) and same_bits(q.detach(), r.detach()), k
    assert not same_bits(on.ema_state.state["p02"], on.p02.detach())
