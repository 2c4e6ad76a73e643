"""Pillow's bilinear ``Image.resize`` of a uint8 image, restated in numpy, one output index and one tap at a time.

Written from the resampling recipe alone (Pillow's two-pass 8-bit path: float64 coefficients per axis, normalised, turned into
22-bit integer taps, a horizontal pass into a uint8 image, a vertical pass over that), independent of the package: nothing
is imported from it.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def coefficients(n_in, n_out):
    """(bounds [n_out, 2] int32 = (xmin, xmax), taps [n_out, ksize] int32, ksize) of one axis.  Python floats are C doubles and
    the interpreter rounds every operation on its own."""
    scale = float(n_in) / float(n_out)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    taps = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = (float(x + xmin) - center + 0.5) * ss
            if a < 0.0:
                a = -a
            wx = 1.0 - a if a < 1.0 else 0.0
            w.append(wx)
            ww = ww + wx
        for x in range(xmax):
            wx = w[x]
            if ww != 0.0:
                wx = wx / ww
            if wx < 0.0:
                taps[xx, x] = int(-0.5 + wx * float(1 << PRECISION_BITS))
            else:
                taps[xx, x] = int(0.5 + wx * float(1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, taps, ksize


def _pass_last_axis(img, n_out):
    """One pass along the last axis of an integer array [..., n_in] -> uint8 [..., n_out]."""
    n_in = img.shape[-1]
    bounds, taps, _ = coefficients(n_in, n_out)
    src = img.astype(np.int64)
    out = np.empty(img.shape[:-1] + (n_out,), np.uint8)
    for xx in range(n_out):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(img.shape[:-1], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(xmax):
            acc = acc + src[..., xmin + x] * int(taps[xx, x])
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(image_hwc, new_h, new_w):
    """``np.asarray(PIL.Image.fromarray(image_hwc).resize((new_w, new_h), BILINEAR))`` for a uint8 [h, w, c] array."""
    img = np.ascontiguousarray(image_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w, _ = img.shape
    if new_w != w:                       # horizontal first, into a uint8 image
        img = _pass_last_axis(img.transpose(0, 2, 1), new_w).transpose(0, 2, 1)
    if new_h != h:
        img = _pass_last_axis(img.transpose(1, 2, 0), new_h).transpose(2, 0, 1)
    return np.ascontiguousarray(img)


def chain(image_hwc, flip, first, crop, final):
    """flip -> optional resize to ``first`` (h, w) -> optional crop (y0, x0, ch, cw) -> resize to ``final`` (h, w)."""
    img = image_hwc[:, ::-1] if flip else image_hwc
    if first is not None:
        img = resize(img, first[0], first[1])
    if crop is not None:
        y0, x0, ch, cw = crop
        img = img[y0:y0 + ch, x0:x0 + cw]
    return resize(img, final[0], final[1])
