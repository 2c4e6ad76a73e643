"""Host side of the fp16 training tail (zira_grad_sqnorm_amp_f32, zira_clip_adamw_amp_f32): the launchers refuse bad
arguments with ``ZIRA_MSDA_EINVAL`` before anything is launched (the pointers below are made-up addresses: a call that got as
far as a launch would not answer EINVAL on a machine without a GPU, and would fault on one with), the workspace size, and
the trainer's switch at its default."""
import ctypes

import pytest

from ziragroundingdino_amd import _lib, optim_tail
from ziragroundingdino_amd.train import ZiraTrainer

EINVAL = 1
N = 70003                        # the GPU tests' bucket: 18 blocks
P = 0x7f0000001000               # "pointers": 16-byte aligned addresses that are never dereferenced on the host


def _blocks(n):
    return (n + optim_tail.CHUNK - 1) // optim_tail.CHUNK


def _amp_bytes(n):
    return 8 * _blocks(n) + 16 + 8 * ((_blocks(n) + 1) // 2)


def _sqnorm_args(**kw):
    a = dict(grad=P, n=N, scale=P + 64, step=P + 128, ws=P + 256, ws_bytes=_amp_bytes(N), stream=None)
    a.update(kw)
    return [a[k] for k in ("grad", "n", "scale", "step", "ws", "ws_bytes", "stream")]


_LRS = (ctypes.c_double * 2)(1e-3, 2e-4)
_ORDER = ("grad", "exp_avg", "exp_avg_sq", "n", "segments", "n_segments", "block_segment", "lrs", "n_groups", "beta1", "beta2",
          "eps", "weight_decay", "max_norm", "scale", "growth_tracker", "step", "growth_factor", "backoff_factor",
          "growth_interval", "norm_out", "found_inf_out", "ws", "ws_bytes", "stream")


def _adamw_args(**kw):
    a = dict(grad=P, exp_avg=P + 0x100000, exp_avg_sq=P + 0x200000, n=N, segments=P + 0x300000, n_segments=6,
             block_segment=P + 0x310000, lrs=_LRS, n_groups=2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, max_norm=0.1,
             scale=P + 0x320000, growth_tracker=P + 0x320010, step=P + 0x320020, growth_factor=2.0, backoff_factor=0.5,
             growth_interval=2000, norm_out=P + 0x320030, found_inf_out=P + 0x320040, ws=P + 0x330000, ws_bytes=_amp_bytes(N),
             stream=None)
    a.update(kw)
    return [a[k] for k in _ORDER]


def test_amp_workspace_bytes():
    lib = _lib.load()
    for n in (1, 4095, 4096, 4097, 8192, 8193, N, optim_tail.MAX_N):
        assert lib.zira_optim_tail_amp_workspace_bytes(n) == _amp_bytes(n)
        assert lib.zira_optim_tail_amp_workspace_bytes(n) % 8 == 0
        # the plain tail's partials, a 16-byte snapshot and one int32 flag per block all fit
        assert lib.zira_optim_tail_amp_workspace_bytes(n) >= lib.zira_optim_tail_workspace_bytes(n) + 16 + 4 * _blocks(n)
    for n in (0, -1, optim_tail.MAX_N + 1):
        assert lib.zira_optim_tail_amp_workspace_bytes(n) == 0


@pytest.mark.parametrize("bad", [
    dict(grad=None), dict(scale=None), dict(step=None), dict(ws=None),
    dict(grad=P + 2), dict(scale=P + 65), dict(step=P + 130), dict(ws=P + 260),
    dict(ws_bytes=_amp_bytes(N) - 1), dict(ws_bytes=8 * _blocks(N)),        # (the plain tail's size is too short)
    dict(n=0), dict(n=-5), dict(n=optim_tail.MAX_N + 1),
], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_sqnorm_amp_refuses(bad):
    lib = _lib.load()
    if "n" in bad and bad["n"] > N:
        bad = dict(bad, ws_bytes=1 << 40)     # (n itself is refused, not a workspace too short for it)
    assert lib.zira_grad_sqnorm_amp_f32(*_sqnorm_args(**bad)) == EINVAL


@pytest.mark.parametrize("bad", [
    dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(segments=None), dict(block_segment=None), dict(lrs=None),
    dict(scale=None), dict(growth_tracker=None), dict(step=None), dict(norm_out=None), dict(found_inf_out=None), dict(ws=None),
    dict(grad=P + 1), dict(exp_avg=P + 0x100002), dict(exp_avg_sq=P + 0x200003), dict(scale=P + 0x320001),
    dict(growth_tracker=P + 0x320012), dict(step=P + 0x320023), dict(norm_out=P + 0x320031), dict(found_inf_out=P + 0x320042),
    dict(ws=P + 0x330004),
    dict(ws_bytes=_amp_bytes(N) - 1), dict(ws_bytes=0),
    dict(n=0), dict(n=-1), dict(n=optim_tail.MAX_N + 1),
    dict(n_segments=0), dict(n_groups=0), dict(n_groups=optim_tail.MAX_GROUPS + 1),
    dict(growth_interval=0), dict(growth_interval=-3),
    dict(growth_factor=0.0), dict(growth_factor=-2.0), dict(growth_factor=float("nan")),
    dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(backoff_factor=float("nan")),
    dict(beta1=1.0), dict(beta2=1.0),
], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_clip_adamw_amp_refuses(bad):
    lib = _lib.load()
    if "n" in bad and bad["n"] > N:
        bad = dict(bad, ws_bytes=1 << 40)
    assert lib.zira_clip_adamw_amp_f32(*_adamw_args(**bad)) == EINVAL


def test_the_switch_is_off_by_default():
    assert ZiraTrainer.native_amp_tail is False
    assert ZiraTrainer.native_tail is False
    assert ZiraTrainer.last_found_inf is None
