"""Pillow's 8-bit resampler restated in numpy / plain Python: the rule include/uwu_hip.h states, the reference of
tests/test_image_folder_cpu.py (against Image.resize itself) and tests/test_image_resize_gpu.py (against the kernels).

Per axis, in Python floats (doubles) with math.sin (libm's):
    scale = in / out; fs = max(scale, 1); support = S * fs; ksize = ceil(support) * 2 + 1
    output xx: center = (xx + 0.5) * scale; xmin = max(int(center - support + 0.5), 0); n = min(int(center + support + 0.5), in) - xmin
               w[x] = filter((x + xmin - center + 0.5) / fs); k[x] = w[x] / sum(w) (ascending x); K[x] = int(k * 2^22 -+ 0.5)
    pixel = clamp((2^21 + sum_x src[xmin + x] * K[x]) >> 22, 0, 255)
The horizontal pass runs first and writes uint8, the vertical pass reads that, a pass whose axis keeps its size is skipped."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}


def coeffs(in_size, out_size, filt):
    """(K int32 [out, ksize], bounds int32 [out, 2] = (xmin, n), ksize) for one axis"""
    fn, S = FILTERS[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ksize = int(math.ceil(support)) * 2 + 1
    K = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[xx, x] = int(k * (1 << PRECISION_BITS) - 0.5) if k < 0 else int(k * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return K, bounds, ksize


def resample_axis(img, axis, out_size, filt, first=0, count=None):
    """img uint8 [H, W, C] -> the outputs first .. first + count - 1 along ``axis`` (0 = vertical, 1 = horizontal), uint8"""
    K, bounds, _ = coeffs(img.shape[axis], out_size, filt)
    count = out_size - first if count is None else count
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((count,) + src.shape[1:], dtype=np.uint8)
    for i in range(count):
        xmin, n = bounds[first + i]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(K[first + i, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31  # (an int32 accumulator holds it)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, filt):
    """Image.resize(size = (width, height), filt) of a uint8 [H, W, C] array"""
    w, h = size
    if img.shape[1] != w:
        img = resample_axis(img, 1, w, filt)
    if img.shape[0] != h:
        img = resample_axis(img, 0, h, filt)
    return np.ascontiguousarray(img)


def resize_crop(img, new_size, window, target_size, filt):
    """the crop (left, top) of size target_size = (width, height) of ``resize(img, new_size, filt)``, computing the window only"""
    (nw, nh), (left, top), (wt, ht) = new_size, window, target_size
    img = resample_axis(img, 1, nw, filt, left, wt) if img.shape[1] != nw else img[:, left:left + wt]
    img = resample_axis(img, 0, nh, filt, top, ht) if img.shape[0] != nh else img[top:top + ht]
    return np.ascontiguousarray(img)
