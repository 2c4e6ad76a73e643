"""Task chain: the loop the reference's driver runs around the training step when it learns one
dataset after another (train_multidatasets.py ``main`` :470-565, ``do_train`` :367-468,
``load_model`` :324-331, ``PeriodicCheckpointer`` :319-322).

    for each task:
        model  <- build_model();  load_state_dict(previous model_final.pth ["model"], strict=False)
        ZiraTrainer(model)        before_train(): only the side branches train
        max_iter x run_step       LR multiplier stepped after every iteration
        after_train(categories)   prompt pool entries + __rep__ merge of every side branch
        <output_dir>/model_final.pth <- {"model": state_dict, "trainer": ..., "iteration": max_iter}

Checkpoints keep the reference's (detectron2 ``Checkpointer``) layout -- a dict with the model's state
dict under ``"model"``, periodic files ``model_{iteration:07d}.pth`` and a ``last_checkpoint`` text file
naming the newest -- and the reference's key names, so either side can continue from the other's files.
``model_final.pth`` is written AFTER the merge (the reference's checkpointer hook saves once more from
``after_train``), which is what makes the next task start from merged twins and 1e-8 branches.

Only what touches the hot path is here: evaluation and the dataset registry of
the reference's driver are not.  The model EMA (ema.py) is, off by default:
``TaskSpec.model_ema`` is the reference's ``train.model_ema``.  So are the metric writers (metrics.py), off by
default: ``TaskSpec.log_period`` is the reference's ``train.log_period`` and writes ``<output_dir>/metrics.json``.
"""
import os
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import ema
from .train import MemoryReplayer, ZiraTrainer


def clean_state_dict(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Drop the ``module.`` prefix a DDP-wrapped model puts on every key (util/utils.py:21-28)."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def multistep_lr_multiplier(decay_iter: int, gamma: float = 0.1) -> Callable[[int], float]:
    """``modified_coco_scheduler(epochs, decay_epochs, base_steps)`` with no warm-up
    (coco_schedule.py:91-125): 1.0 for iterations < decay_iter, ``gamma`` from there on."""
    return lambda it: 1.0 if it < decay_iter else gamma


@dataclass
class TaskSpec:
    """One task config of the reference (test_odinw13_softfreeze/for_train/test_*.py)."""
    name: str
    categories_names: Sequence[str]
    data: Callable[[int], Iterable]          # start_iter -> iterator of minibatches (endless or >= max_iter long)
    max_iter: int
    output_dir: str
    lr: float = 1e-3
    weight_decay: float = 1e-4
    clip_max_norm: Optional[float] = 0.1
    clip_norm_type: float = 2.0
    lr_multiplier: Optional[Callable[[int], float]] = None   # default: x0.1 after 40 % (10 epochs, decay at 4)
    checkpoint_period: Optional[int] = None                  # default: max_iter (the configs' 10 epochs)
    batch_size_scale: int = 1                                # optimizer step every k iterations (train_multidatasets.py:192-199)
    model_ema: Optional[dict] = None                         # train.model_ema: None = off, or dict(decay=0.999, device="")
    use_ema_weights_for_eval_only: bool = False              # (:338, :534) evaluate a finished task under the averaged weights
    log_period: Optional[int] = None                         # train.log_period (20): <output_dir>/metrics.json every so many iterations; None = off
    replay: bool = False                                     # --replay (:496-506): a text-only stage of model.replay_memory() iterations; ``data`` is not read

    def multiplier(self) -> Callable[[int], float]:
        return self.lr_multiplier or multistep_lr_multiplier((self.max_iter * 4) // 10)


def load_model(build_model: Callable[[], torch.nn.Module], checkpoint_path: Optional[str], device="cpu"):
    """Fresh model + the previous task's weights.  ``strict=False`` as in the reference: a checkpoint
    from before ZiRa has no side-branch keys, and prompt pool entries create themselves on load."""
    model = build_model()
    if checkpoint_path:
        checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        model.load_state_dict(clean_state_dict(checkpoint["model"]), strict=False)
    return model.to(device).train()       # the reference trains with the whole model in train mode (:330)


def _is_main(group) -> bool:
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank(group) == 0


def _barrier(group):
    if dist.is_available() and dist.is_initialized():
        dist.barrier(group=group)


def save_checkpoint(output_dir: str, name: str, model, trainer: ZiraTrainer, iteration: int) -> str:
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, name + ".pth")
    tmp = path + ".tmp"
    # ``may_get_ema_checkpointer`` (:428-429): the checkpointer stores ``ema_state.state_dict()`` beside ``"model"``
    extra = ema.may_get_ema_checkpointer(model, enabled=getattr(trainer, "model_ema", None) is not None)
    extra = {k: {n: v.detach().cpu() for n, v in obj.state_dict().items()} for k, obj in extra.items()}
    torch.save({"model": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "trainer": {"iteration": iteration, "optimizer": trainer.optimizer.state_dict()},
                "iteration": iteration, **extra}, tmp)
    os.replace(tmp, path)               # a killed run never leaves a half-written file under the final name
    with open(os.path.join(output_dir, "last_checkpoint"), "w") as f:
        f.write(name + ".pth")
    return path


def _resume(spec: TaskSpec, model, trainer: ZiraTrainer) -> int:
    """``checkpointer.resume_or_load(resume=True)`` (:461-466): continue after the iteration the newest
    periodic checkpoint of THIS task stored.  Returns the iteration to start at."""
    marker = os.path.join(spec.output_dir, "last_checkpoint")
    if not os.path.exists(marker):
        return 0
    with open(marker) as f:
        path = os.path.join(spec.output_dir, f.read().strip())
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(clean_state_dict(checkpoint["model"]), strict=False)
    trainer._bind()
    trainer.optimizer.load_state_dict(checkpoint["trainer"]["optimizer"])
    for key, obj in ema.may_get_ema_checkpointer(model, enabled=getattr(trainer, "model_ema", None) is not None).items():
        if key in checkpoint:       # (moved to the device and packed before the first step: ZiraTrainer.ema_before_train)
            obj.load_state_dict(checkpoint[key])
    return int(checkpoint["trainer"]["iteration"]) + 1


def _check_matching(model, process_group=None):
    """The device-side matcher records what the reference stops on at once (scipy's ValueError for an
    infeasible -- inf / NaN -- cost matrix, ``generalized_box_iou``'s xyxy assertion:
    matcher/matcher.py:147, util/box_ops.py:51-52) as device flags and goes on with dummy assignments.
    Read them back here so that a diverged run ends before a checkpoint is written or merged.  With several ranks the
    verdict is all-reduced (MAX) first: every rank raises together instead of one raising and the others hanging in
    their next collective until the RCCL timeout."""
    criterion = getattr(model, "criterion", None)
    matcher = getattr(criterion, "matcher", None)
    err = None
    if matcher is not None and hasattr(matcher, "check"):
        try:
            matcher.check()
        except (AssertionError, ValueError) as exc:
            err = exc
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        dev = next(model.parameters()).device
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32,
                            device=dev if dist.get_backend(process_group) == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=process_group)
        if err is None and int(flag.item()):
            err = RuntimeError("device-side matching failed on another rank (infeasible cost matrix or boxes not in xyxy order)")
    if err is not None:
        raise err


def run_task(spec: TaskSpec, build_model, init_checkpoint: Optional[str], device="cpu", process_group=None,
             resume=False, on_step=None, evaluate=None):
    """``do_train`` for one task; returns the path of its ``model_final.pth``.  ``evaluate``: a callable
    ``(model, spec) -> dict`` run on the merged model (``do_test`` after training, train_multidatasets.py:338-364, e.g.
    ``evaluation.inference_on_dataset`` over the task's test set); the return value is then ``(path, its result)``.  With
    ``spec.model_ema`` it runs a second time under the averaged weights (``apply_model_ema_and_restore``, :356-364) and that
    result is the first one's ``"ema"`` entry (the reference's ``ret.update(ema_ret)`` overwrites the plain figures instead).

    A replay spec (``spec.replay``, the reference's ``--replay`` stage behind the last task) builds no loader and learns no class:
    ``max_iter`` iterations of ``MemoryReplayer`` (``model.replay_memory()`` + the trainer's tail), then ``model.after_train()``
    -- the merge -- and ``model_final.pth``.  The reference's ``MemoryReplayer.after_train`` runs hooks only and saves unmerged
    branches; merging keeps this chain's invariant that every ``model_final.pth`` starts the next task from merged twins.  No
    ``add_cls_prompt`` there."""
    final = os.path.join(spec.output_dir, "model_final.pth")
    if resume and os.path.exists(final):
        if evaluate is None:
            return final
        model = load_model(build_model, final, device)
        if spec.model_ema is not None:
            ema.may_build_model_ema(model, enabled=True)
            checkpoint = torch.load(final, map_location="cpu", weights_only=False)
            if "ema_state" in checkpoint:
                model.ema_state.load_state_dict(checkpoint["ema_state"])
                model.ema_state.to(device)
        return final, _evaluate(evaluate, model, spec)
    model = load_model(build_model, init_checkpoint, device)
    if getattr(model, "use_prompt_tuning", False) and not spec.replay:
        # prompt tuning trains the pool entries of this task's classes: they exist before the trainer builds its gradient bucket
        # and optimizer over the trainable tensors (the reference's do_train, train_multidatasets.py:393-394)
        model.add_cls_prompt(list(spec.categories_names))
    writers = []
    if spec.log_period is not None and _is_main(process_group):      # (:436-459: the writers are the main process's)
        from . import metrics

        writers = [metrics.CommonMetricPrinter(spec.max_iter), metrics.JSONWriter(os.path.join(spec.output_dir, "metrics.json"))]
    trainer_class = MemoryReplayer if spec.replay else ZiraTrainer
    trainer = trainer_class(model, lr=spec.lr, weight_decay=spec.weight_decay, clip_max_norm=spec.clip_max_norm,
                            clip_norm_type=spec.clip_norm_type, process_group=process_group,
                            batch_size_scale=spec.batch_size_scale, model_ema=spec.model_ema,
                            metrics=None if spec.log_period is None else dict(period=spec.log_period, writers=writers))
    base_lrs = [g["lr"] for g in trainer.optimizer.param_groups]   # before a resume: a checkpoint stores the
    start_iter = _resume(spec, model, trainer) if resume else 0    # MULTIPLIED rates of the iteration it was taken at
    trainer.iter = start_iter             # (the reference's step rule, iter % batch_size_scale == 0, counts from here)
    assert len(base_lrs) == len(trainer.optimizer.param_groups)
    multiplier = spec.multiplier()
    period = spec.checkpoint_period or spec.max_iter
    batches = None if spec.replay else iter(spec.data(start_iter))
    for it in range(start_iter, spec.max_iter):
        for g, base in zip(trainer.optimizer.param_groups, base_lrs):
            g["lr"] = base * multiplier(it)
        loss_dict = trainer.run_step() if spec.replay else trainer.run_step(next(batches))
        if on_step is not None:
            on_step(spec, it, loss_dict)
        if (it + 1) % period == 0:
            _check_matching(model, process_group)        # before anything is written: one host sync per checkpoint period
            if _is_main(process_group):
                save_checkpoint(spec.output_dir, "model_%07d" % it, model, trainer, it)
    for writer in writers:
        writer.close()
    _check_matching(model, process_group)                # ... and before the side branches are merged into the weights
    trainer.after_train([] if spec.replay else list(spec.categories_names))      # (replay learns no class: the merge only)
    if _is_main(process_group):
        save_checkpoint(spec.output_dir, "model_final", model, trainer, spec.max_iter)
    _barrier(process_group)               # every rank loads this file at the start of the next task
    return final if evaluate is None else (final, _evaluate(evaluate, model, spec))


def _evaluate(evaluate, model, spec: TaskSpec):
    """``do_test`` (:338-365).  EMA off: ``evaluate(model, spec)`` as it is."""
    if spec.model_ema is None or not getattr(model, "ema_state", None) or not model.ema_state.has_inited():
        return evaluate(model, spec)
    if spec.use_ema_weights_for_eval_only:      # (:534-535) apply without restore, then evaluate
        ema.apply_model_ema(model)
        return evaluate(model, spec)
    result = evaluate(model, spec)
    with ema.apply_model_ema_and_restore(model):
        ema_result = evaluate(model, spec)
    result = dict(result)
    result["ema"] = ema_result
    return result


def run_tasks(specs: Sequence[TaskSpec], build_model, init_checkpoint: Optional[str] = None, device="cpu",
              process_group=None, resume=False, on_step=None, evaluate=None) -> List:
    """The task loop of ``main`` (:531-560): each task starts from the previous one's
    ``model_final.pth``.  Returns the list of final checkpoints, one per task -- with ``evaluate`` (see ``run_task``)
    the list of ``(checkpoint, result)`` pairs."""
    finals = []
    for spec in specs:
        done = run_task(spec, build_model, init_checkpoint, device, process_group, resume, on_step, evaluate)
        init_checkpoint = done if evaluate is None else done[0]
        finals.append(done)
    return finals
