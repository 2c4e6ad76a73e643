"""The padded full-size fixture (tests/golden/gen_fullsize_padded_golden.py) on the CPU: the inputs it was made from have the
intended geometry, and the stored file holds what the GPU pin (test_padded_fullsize_gpu.py) reads."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from gen_fullsize_golden import SHAPES, make_inputs  # noqa: E402
from gen_fullsize_padded_golden import make_padded_inputs  # noqa: E402


def _nearest_valid(n_out, n_in, n_valid):
    # F.interpolate(mode="nearest"): output index i reads input floor(i * n_in / n_out)
    return sum(1 for i in range(n_out) if (i * n_in) // n_out < n_valid)


def test_padded_inputs_geometry():
    srcs, poss, masks, text, tmask, pid, may, gos = make_padded_inputs()
    base = make_inputs()
    for a, b in zip(srcs + poss + [text] + gos, base[0] + base[1] + [base[3]] + base[7]):
        assert torch.equal(a, b)                      # only the masks differ from the unpadded pin
    for m, (h, w) in zip(masks, SHAPES):
        assert m.shape == (2, h, w) and not m[0].any()
        vh, vw = _nearest_valid(h, 800, 640), _nearest_valid(w, 1333, 1066)
        assert 0 < vh < h and 0 < vw < w, (h, w, vh, vw)
        want = torch.ones(h, w, dtype=torch.bool)
        want[:vh, :vw] = False                        # valid: the top-left vh x vw block
        assert torch.equal(m[1], want), (h, w)
    assert [_nearest_valid(h, 800, 640) for h, _ in SHAPES] == [80, 40, 20, 11]
    assert [_nearest_valid(w, 1333, 1066) for _, w in SHAPES] == [134, 68, 34, 17]
    assert tmask[0].all() and int(tmask[1].sum()) == 20 and tmask[1, :20].all()
    assert (pid[1, 20:] == 0).all() and torch.equal(pid[0], base[5][0]) and torch.equal(pid[1, :20], base[5][1, :20])
    n = may.shape[-1]
    pad = may[1, 20:]
    assert torch.equal(pad, torch.eye(n, dtype=torch.bool)[20:])   # padded tokens see only themselves
    assert not may[1, :20, 20:].any() and torch.equal(may[0], base[6][0])


def test_padded_fixture_keys():
    g = torch.load(os.path.join(HERE, "golden", "full_transformer_padded.pt"), weights_only=False)
    ref = torch.load(os.path.join(HERE, "golden", "full_transformer.pt"), weights_only=False)
    assert set(g) == set(ref) | {"strides"}
    assert g["salt"] == ref["salt"] and g["kwargs"] == ref["kwargs"] and g["param_names"] == ref["param_names"]
    assert g["topk_proposals"].shape == (2, 900)
    st = g["strides"]
    assert g["hs_last"].shape == (2, 900, 256 // st["hs_last_channels"])
    assert g["grad_src3"].shape == (2, 256 // st["grad_src3_channels"], 13, 21)
    assert torch.isfinite(g["total"]) and torch.isfinite(g["grad_text"]).all()
    assert os.path.getsize(os.path.join(HERE, "golden", "full_transformer_padded.pt")) < 1 << 20
