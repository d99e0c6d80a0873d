"""Restatement of PIL's Image.resize(..., Image.BILINEAR) for uint8 RGB frames (Pillow's two-pass resample in 8-bit fixed point), in
numpy and Python doubles: the reference of the device Resize (csrc/resize.h).  test_device_resize.py pins it to Pillow bit for bit.

Per axis (n_in -> n_out): scale = n_in / n_out, fs = max(scale, 1), support = fs, ksize = int(ceil(support)) * 2 + 1; per output xx:
center = (xx + 0.5) * scale, xmin = max(0, int(center - support + 0.5)), xmax = min(n_in, int(center + support + 0.5)),
w[x] = tri((x + xmin - center + 0.5) / fs), k = w / sum(w), K = int(0.5 + k * 2^22).  A pass: clamp((2^21 + sum K * pixel) >> 22).
Horizontal first, rounded to uint8, then vertical; an axis whose size does not change has no pass."""
import math

import numpy as np

BITS = 22


def coeffs(n_in, n_out):
    """-> (xmin [n_out], taps [n_out], K [n_out, ksize] int64)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmins, taps, K = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        w = []
        for x in range(n):
            a = abs((x + xmin - center + 0.5) / fs)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            K[xx, x] = int(-0.5 + k * (1 << BITS)) if k < 0 else int(0.5 + k * (1 << BITS))
        xmins[xx], taps[xx] = xmin, n
    return xmins, taps, K


def one_pass(img, n_out, axis):
    """img uint8 [..., H, W, 3]; resample `axis` (-3 rows, -2 columns) to n_out"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    xmins, taps, K = coeffs(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx in range(n_out):
        n = int(taps[xx])
        k = K[xx, :n].reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (BITS - 1)) + (k * src[xmins[xx]:xmins[xx] + n]).sum(axis=0)
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31  # Pillow accumulates in 32-bit integers
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(img, H, W):
    """uint8 [..., h, w, 3] -> uint8 [..., H, W, 3], = Image.fromarray(frame).resize((W, H), Image.BILINEAR) per frame"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    return np.ascontiguousarray(one_pass(one_pass(img, W, -2), H, -3))
