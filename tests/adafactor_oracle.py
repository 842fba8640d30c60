"""transformers.optimization.Adafactor.step in numpy float64, one function per step over a list of tensors.

A tensor is a dict of float64 arrays: ``p`` and ``g`` ([R, C] or 1-D), and its state ``row`` [R] / ``col`` [C] (factored: two or
more dimensions) or ``v`` (1-D), plus ``m`` with ``beta1``.  ``g`` is the raw gradient; ``gscale`` = pre_scale * clip coefficient
multiplies it first, as the fused kernels do.
"""
import math

import numpy as np


def view2d(shape):
    """the [R, C] view of a stored tensor of two or more dimensions; None for a 1-D one"""
    shape = tuple(int(d) for d in shape)
    return (shape[0], int(np.prod(shape[1:]))) if len(shape) >= 2 else None


def new_state(p, beta1=None):
    st = {}
    if p.ndim >= 2:
        st["row"], st["col"] = np.zeros(p.shape[0]), np.zeros(p.shape[1])
    else:
        st["v"] = np.zeros(p.shape)
    if beta1 is not None:
        st["m"] = np.zeros(p.shape)
    return st


def rms(x):
    return float(np.sqrt(np.sum(x * x)) / math.sqrt(x.size))


def step_size(step, lr=None, relative_step=True, warmup_init=False):
    if not relative_step:
        return float(lr)
    return min(1e-6 * step if warmup_init else 1e-2, 1.0 / math.sqrt(step))


def adafactor_step(tensors, step, *, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None,
                   weight_decay=0.0, scale_parameter=True, relative_step=True, warmup_init=False, gscale=1.0):
    """One step (``step`` is 1-based) of every tensor: a new list of dicts with ``p`` and the state advanced (``g`` kept) and, for
    the tests' own assertions, ``rms_u`` (RMS of the update before the clip) and ``rms_p`` (RMS of ``p`` before the update)."""
    beta2t = 1.0 - math.pow(step, decay_rate)
    lr_t = step_size(step, lr, relative_step, warmup_init)
    out = []
    for t in tensors:
        p = np.asarray(t["p"], np.float64)
        g = np.asarray(t["g"], np.float64) * float(gscale)
        n = dict(g=t["g"])
        alpha = lr_t * (max(eps[1], rms(p)) if scale_parameter else 1.0)
        U = g * g + eps[0]
        if p.ndim >= 2:
            row = beta2t * np.asarray(t["row"], np.float64) + (1.0 - beta2t) * U.mean(axis=1)
            col = beta2t * np.asarray(t["col"], np.float64) + (1.0 - beta2t) * U.mean(axis=0)
            u = g * ((1.0 / np.sqrt(row / row.mean()))[:, None] * (1.0 / np.sqrt(col))[None, :])
            n["row"], n["col"] = row, col
        else:
            v = beta2t * np.asarray(t["v"], np.float64) + (1.0 - beta2t) * U
            u = g / np.sqrt(v)
            n["v"] = v
        n["rms_u"], n["rms_p"] = rms(u), rms(p)
        u = u / max(1.0, n["rms_u"] / clip_threshold)
        u = u * alpha
        if beta1 is not None:
            u = n["m"] = beta1 * np.asarray(t["m"], np.float64) + (1.0 - beta1) * u
        if weight_decay != 0:
            p = p - weight_decay * alpha * p
        n["p"] = p - u
        out.append(n)
    return out
