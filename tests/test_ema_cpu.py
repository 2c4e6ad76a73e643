"""The model EMA (ziragroundingdino_amd/ema.py) without a GPU: ``update_reference`` against what the reference's own
``EMAUpdater`` recorded (tests/golden/ema_zira_slice.pt, the same torch CPU ops: bit for bit), the ``EMAState`` round trips,
the trainer and the task chain carrying it, and the segment planning against a loop over every flat element."""
import itertools
import os
import sys

import pytest
import torch
from torch import nn

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from gen_ema_golden import DECAY, SIZES, STEPS, Tiny, model_state, set_step, tiny_module  # noqa: E402

from ziragroundingdino_amd import ema, tasks  # noqa: E402
from ziragroundingdino_amd.train import ZiraTrainer  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "ema_zira_slice.pt"), weights_only=False)


def same_bits(a, b):
    """Equal dtype, shape and bits (signed zeros and NaNs included)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(view), b.contiguous().view(view))
    return torch.equal(a, b)


def assert_state_is(state, want, what):
    assert list(state) == list(want), what
    for k in want:
        assert same_bits(state[k].cpu(), want[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("through", ["update_reference", "EMAUpdater"])
def test_eight_steps_reproduce_the_reference_bit_for_bit(golden, through):
    """fp32 parameters, the fp16, the int64 (truncating) and the bool buffer, after every step."""
    assert golden["decay"] == DECAY and golden["sizes"] == SIZES and len(golden["steps"]) == STEPS
    model = tiny_module()
    state = ema.EMAState()
    updater = ema.EMAUpdater(state, decay=DECAY, device="")
    updater.init_state(model)
    assert list(state.state_dict()) == golden["keys"]
    for k in range(1, STEPS + 1):
        set_step(model, k)
        if through == "EMAUpdater":
            updater.update(model)        # CPU tensors: the kernel declines them all
        else:
            ema.update_reference(state, model, DECAY)
        assert_state_is(state.state_dict(), golden["steps"][k - 1], "step %d" % k)
    assert golden["steps"][-1]["count"].dtype == torch.int64 and golden["steps"][-1]["flag"].dtype == torch.bool


def _at_step_8(golden):
    model = tiny_module()
    for k in range(1, STEPS + 1):
        set_step(model, k)
    state = ema.EMAState()
    state.load_state_dict({k: v.clone() for k, v in golden["steps"][-1].items()})
    return model, state


def test_state_dict_round_trip(golden):
    _, state = _at_step_8(golden)
    assert state.has_inited() and state.device == torch.device("cpu")
    other = ema.EMAState()
    assert not other.has_inited() and other.device is None
    ret = other.load_state_dict(state.state_dict())
    assert ret.missing_keys == [] and ret.unexpected_keys == []
    assert_state_is(other.state_dict(), golden["steps"][-1], "loaded")
    assert other.to("cpu") is other
    assert_state_is(other.state_dict(), golden["steps"][-1], "after to()")
    assert not other.clear().has_inited()


def test_apply_and_restore(golden):
    model, state = _at_step_8(golden)
    before = model_state(model)
    with state.apply_and_restore(model):
        inside = model_state(model)
    after = model_state(model)
    params = [k for k, _ in model.named_parameters()]
    for k in params:
        assert same_bits(inside[k], golden["steps"][-1][k]), k
    for k, v in golden["applied_buffers"].items():
        assert same_bits(inside[k], v), k
    for k, v in golden["restored_buffers"].items():
        assert same_bits(after[k], v), k
    for k in before:
        assert same_bits(after[k], before[k]), k
    assert_state_is(state.state_dict(), golden["steps"][-1], "the state after the context")
    # the module functions go the same way
    model.ema_state = state
    with ema.apply_model_ema_and_restore(model):
        assert all(same_bits(getattr(model, k).detach(), golden["steps"][-1][k]) for k in params)
    assert all(same_bits(getattr(model, k).detach(), before[k]) for k in params)
    old = ema.apply_model_ema(model, save_current=True)
    assert all(same_bits(getattr(model, k).detach(), golden["steps"][-1][k]) for k in params)
    assert all(same_bits(old.state[k], before[k]) for k in before)
    twin = state.get_ema_model(model)
    assert twin is not model and same_bits(twin.p02.detach(), golden["steps"][-1]["p02"])


class Trainable(Tiny):
    """The fixture's module with what ``ZiraTrainer`` and the task chain ask of a model."""

    def before_train(self):
        pass

    def after_train(self):
        pass

    def add_cls_prompt(self, names):
        for name in names:
            self.register_parameter("prompt_" + name, nn.Parameter(torch.full((3,), 0.25, device=self.p00.device)))

    def load_state_dict(self, state_dict, strict=True):
        self.add_cls_prompt([k[7:] for k in state_dict if k.startswith("prompt_") and not hasattr(self, k)])   # as the prompt pool does
        return super().load_state_dict(state_dict, strict=strict)

    def forward(self, data):
        loss = sum((p * p).mean() for name, p in self.named_parameters() if name.startswith("p"))
        return {"loss_sq": loss * data}


@pytest.mark.parametrize("batch_size_scale", [1, 2])
def test_trainer_state_equals_update_reference_by_hand(batch_size_scale):
    """The state starts from the model before the first step and is updated after EVERY run_step, accumulation iterations
    (no optimizer step) included: every entry equals ``update_reference`` run by hand beside a trainer without EMA."""
    a, b = Trainable().train(), Trainable().train()
    trainer = ZiraTrainer(a, lr=1e-2, tuned_gemms=False, batch_size_scale=batch_size_scale, model_ema=dict(decay=0.9, device=""))
    plain = ZiraTrainer(b, lr=1e-2, tuned_gemms=False, batch_size_scale=batch_size_scale)
    assert isinstance(a.ema_state, ema.EMAState) and not a.ema_state.has_inited()
    by_hand = ema.EMAState.FromModel(b)
    for it in range(4):
        trainer.run_step(1.0 + it)
        plain.run_step(1.0 + it)
        ema.update_reference(by_hand, b, 0.9)
        assert_state_is(a.ema_state.state_dict(), dict(by_hand.state_dict()), "iteration %d" % it)
        assert not same_bits(a.ema_state.state["p02"], a.p02.detach())
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert same_bits(p.detach(), q.detach()), k      # the average does not disturb the step
    assert float((a.p02.detach() - Tiny().p02.detach()).abs().max()) > 0


def test_without_model_ema_nothing_is_there(tmp_path):
    model = Trainable().train()
    trainer = ZiraTrainer(model, tuned_gemms=False)
    trainer.run_step(1.0)
    assert not hasattr(model, "ema_state") and trainer.model_ema is None
    path = tasks.save_checkpoint(str(tmp_path), "model_0000000", model, trainer, 0)
    assert set(torch.load(path, weights_only=False)) == {"model", "trainer", "iteration"}
    assert ema.may_get_ema_checkpointer(model, enabled=False) == {}
    ema.may_build_model_ema(model, enabled=False)
    assert not hasattr(model, "ema_state")


def test_checkpoint_carries_ema_state_and_resume_restores_it(golden, tmp_path):
    model = Trainable().train()
    trainer = ZiraTrainer(model, lr=1e-2, tuned_gemms=False, model_ema=dict(decay=DECAY))
    for _ in range(2):
        trainer.run_step(1.0)
    path = tasks.save_checkpoint(str(tmp_path), "model_0000001", model, trainer, 1)
    checkpoint = torch.load(path, weights_only=False)
    assert set(checkpoint) == {"model", "trainer", "iteration", "ema_state"}
    assert list(checkpoint["ema_state"]) == golden["keys"]        # the reference's names, in its order
    assert_state_is(checkpoint["ema_state"], dict(model.ema_state.state_dict()), "saved")
    # a fresh model and trainer continue from it
    spec = tasks.TaskSpec("t", [], lambda start: itertools.repeat(1.0), 4, str(tmp_path), model_ema=dict(decay=DECAY))
    model2 = Trainable().train()
    trainer2 = ZiraTrainer(model2, lr=1e-2, tuned_gemms=False, model_ema=spec.model_ema)
    assert tasks._resume(spec, model2, trainer2) == 2
    assert_state_is(model2.ema_state.state_dict(), checkpoint["ema_state"], "resumed")
    trainer.run_step(1.0)
    trainer2.run_step(1.0)      # (the loaded state is kept, not re-initialised from the model)
    for k, _ in model.named_parameters():
        assert same_bits(model2.ema_state.state[k], model.ema_state.state[k]), k


def test_run_task_evaluates_a_second_time_under_the_average(tmp_path):
    def evaluate(model, spec):
        return {"p02_sum": float(model.p02.detach().double().sum()), "n_tensors": len(list(model.named_parameters()))}

    def spec(name, **kw):
        return tasks.TaskSpec(name, ["fish"], lambda start: itertools.repeat(1.0), 3, str(tmp_path / name), lr=1e-2, **kw)

    _, plain = tasks.run_task(spec("off"), Trainable, None, evaluate=evaluate)
    _, both = tasks.run_task(spec("on", model_ema=dict(decay=0.5)), Trainable, None, evaluate=evaluate)
    assert set(plain) == {"p02_sum", "n_tensors"} and set(both) == {"p02_sum", "n_tensors", "ema"}
    assert {k: both[k] for k in plain} == plain                    # the plain figures are the ones EMA-off gives
    assert both["ema"]["p02_sum"] != plain["p02_sum"] and both["ema"]["n_tensors"] == plain["n_tensors"]
    assert "ema_state" in torch.load(str(tmp_path / "on" / "model_final.pth"), weights_only=False)
    assert "prompt_fish" in torch.load(str(tmp_path / "on" / "model_final.pth"), weights_only=False)["ema_state"]
    _, only = tasks.run_task(spec("only", model_ema=dict(decay=0.5), use_ema_weights_for_eval_only=True), Trainable, None,
                             evaluate=evaluate)
    assert only == both["ema"]
    # a finished task evaluated again from its files
    _, again = tasks.run_task(spec("on", model_ema=dict(decay=0.5)), Trainable, None, resume=True, evaluate=evaluate)
    assert again == both


def _brute_force(numels, chunk, align):
    owner, starts = [], []
    for s, x in enumerate(numels):
        while len(owner) % align:
            owner.append(-1)            # a gap element belongs to no segment
        starts.append(len(owner))
        owner += [s] * x
    return owner, starts


@pytest.mark.parametrize("numels", [SIZES, [4096], [4096, 1], [4095, 2, 4095, 8192, 7], [1] * 3000, [3, 12285, 1]])
def test_segment_planning_matches_a_loop_over_the_elements(numels):
    chunk, align = ema.CHUNK, ema.ALIGN
    starts, block_segment, n = ema.plan_segments(numels)
    owner, want_starts = _brute_force(numels, chunk, align)
    assert starts == want_starts and n == len(owner) and all(s % align == 0 for s in starts)
    assert len(block_segment) == (n + chunk - 1) // chunk
    for b, s in enumerate(block_segment):      # the segment of the block's first element, or the next one behind a gap
        assert s == next(o for o in owner[b * chunk:] if o >= 0)
    # the kernel's walk from there reaches every owned element exactly once and no gap element
    seen = [0] * n
    for b, s in enumerate(block_segment):
        cs, ce = b * chunk, min(n, (b + 1) * chunk)
        while s < len(numels) and starts[s] < ce:
            for i in range(max(starts[s], cs), min(starts[s] + numels[s], ce)):
                assert owner[i] == s
                seen[i] += 1
            s += 1
    assert seen == [1 if o >= 0 else 0 for o in owner]


def test_block_index_of_a_partial_table():
    """A table that names only some of the layout's segments (a tensor the kernel no longer serves): blocks inside the hole
    point at the next segment, blocks behind the last one at the end of the table."""
    starts, numels = [0, 3 * 4096 + 8], [5, 10]
    idx = ema.block_index(starts, numels, 5 * 4096)
    assert idx == [0, 1, 1, 1, 2]


def test_planning_constants_are_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(ema.__file__)))
    with open(os.path.join(root, "include", "zira_msda.h")) as f:
        header = f.read()
    assert "#define ZIRA_EMA_CHUNK %d\n" % ema.CHUNK in header
    assert "#define ZIRA_EMA_MAX_N %dll\n" % ema.MAX_N in header
    assert ema.MAX_N >= 1 << 30


def test_entry_points_decline_unserved_sizes_without_a_gpu():
    """n = 0, n above the limit, null pointers: the "not served" code, and nothing is launched (there is no device here)."""
    from ziragroundingdino_amd import _lib

    lib = _lib.load()
    table = torch.zeros(3, dtype=torch.int64)
    idx = torch.zeros(1, dtype=torch.int32)
    buf = torch.zeros(4)
    for n in (0, -1, ema.MAX_N + 1):
        assert lib.zira_ema_update_f32(buf.data_ptr(), n, table.data_ptr(), 1, idx.data_ptr(), 0.9, 0.1, 1, None) == 1
        assert lib.zira_ema_swap_f32(buf.data_ptr(), n, table.data_ptr(), 1, idx.data_ptr(), None) == 1
        assert lib.zira_ema_copy_f32(buf.data_ptr(), n, table.data_ptr(), 1, idx.data_ptr(), 0, None) == 1
    assert lib.zira_ema_update_f32(None, 4, table.data_ptr(), 1, idx.data_ptr(), 0.9, 0.1, 1, None) == 1
    assert lib.zira_ema_swap_f32(buf.data_ptr(), 4, table.data_ptr(), 0, idx.data_ptr(), None) == 1
