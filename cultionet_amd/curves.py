"""The two interpolators behind the random curves of the series augmenters (``cultionet_amd.augment``), in numpy only:
``tsaug``'s ``TimeWarp`` draws its warp through ``scipy.interpolate.PchipInterpolator`` and its ``Drift`` through
``scipy.interpolate.CubicSpline``; the package and its GPU tests must run where scipy is not installed.

  pchip(x, y, xq)          monotone cubic Hermite interpolant, the derivative rule of PchipInterpolator
  cubic_spline(x, y, xq)   C2 cubic spline with CubicSpline's default ``bc_type="not-a-knot"``

``x`` [n] strictly increasing knots, ``y`` [..., n] values (any leading axes), ``xq`` [m] query points inside
``[x[0], x[-1]]`` -> [..., m], float64. tests/test_curves.py holds both to scipy within 1e-12.
"""
from __future__ import annotations

import numpy as np


def _prepare(x, y, xq):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64)
    if x.ndim != 1 or x.size < 2 or y.shape[-1] != x.size or not (np.diff(x) > 0).all():
        raise ValueError("x must hold at least two strictly increasing knots, y one value per knot along its last axis")
    if xq.ndim != 1 or (xq.size and (xq.min() < x[0] or xq.max() > x[-1])):
        raise ValueError("xq must be one axis of points inside [x[0], x[-1]]")
    return x, y, xq


def _hermite(x, y, d, xq):
    """The piecewise cubic with values y and derivatives d at the knots, at xq: scipy's power form in (xq - x[i])."""
    i = np.clip(np.searchsorted(x, xq, side="right") - 1, 0, x.size - 2)
    h = np.diff(x)[i]
    m = (y[..., i + 1] - y[..., i]) / h
    t = xq - x[i]
    c3 = (d[..., i] + d[..., i + 1] - 2.0 * m) / (h * h)
    c2 = (3.0 * m - 2.0 * d[..., i] - d[..., i + 1]) / h
    return ((c3 * t + c2) * t + d[..., i]) * t + y[..., i]


def _pchip_end(h0, h1, m0, m1):
    """One-sided three-point derivative estimate, shape preserving (PchipInterpolator._edge_case)."""
    d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    d = np.where(np.sign(d) != np.sign(m0), 0.0, d)
    return np.where((np.sign(m0) != np.sign(m1)) & (np.abs(d) > 3.0 * np.abs(m0)), 3.0 * m0, d)


def pchip(x, y, xq) -> np.ndarray:
    x, y, xq = _prepare(x, y, xq)
    h = np.diff(x)
    m = np.diff(y, axis=-1) / h
    d = np.zeros_like(y)
    if x.size == 2:
        d[...] = m
        return _hermite(x, y, d, xq)
    # interior knots: the weighted harmonic mean of the two secant slopes, 0 where they differ in sign or one is 0
    w1, w2 = 2.0 * h[1:] + h[:-1], h[1:] + 2.0 * h[:-1]
    m0, m1 = m[..., :-1], m[..., 1:]
    flat = (np.sign(m0) != np.sign(m1)) | (m0 == 0.0) | (m1 == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (w1 + w2) / (w1 / m0 + w2 / m1)
    d[..., 1:-1] = np.where(flat, 0.0, mean)
    d[..., 0] = _pchip_end(h[0], h[1], m[..., 0], m[..., 1])
    d[..., -1] = _pchip_end(h[-1], h[-2], m[..., -1], m[..., -2])
    return _hermite(x, y, d, xq)


def cubic_spline(x, y, xq) -> np.ndarray:
    x, y, xq = _prepare(x, y, xq)
    n = x.size
    h = np.diff(x)
    m = np.diff(y, axis=-1) / h
    if n == 2:
        d = np.repeat(m, 2, axis=-1)
        return _hermite(x, y, d, xq)
    # the knot derivatives s solve A s = b: continuity of the second derivative at the interior knots, and the third
    # derivative continuous across the first and the last interior knot (with three knots: one parabola through them)
    A = np.zeros((n, n))
    b = np.empty_like(y)
    k = np.arange(1, n - 1)
    A[k, k - 1], A[k, k], A[k, k + 1] = h[1:], 2.0 * (h[:-1] + h[1:]), h[:-1]
    b[..., 1:-1] = 3.0 * (h[1:] * m[..., :-1] + h[:-1] * m[..., 1:])
    if n == 3:
        A[0, :2] = 1.0
        A[2, 1:] = 1.0
        b[..., 0], b[..., 2] = 2.0 * m[..., 0], 2.0 * m[..., 1]
    else:
        a, z = x[2] - x[0], x[-1] - x[-3]
        A[0, 0], A[0, 1] = h[1], a
        A[-1, -1], A[-1, -2] = h[-2], z
        b[..., 0] = ((h[0] + 2.0 * a) * h[1] * m[..., 0] + h[0] ** 2 * m[..., 1]) / a
        b[..., -1] = (h[-1] ** 2 * m[..., -2] + (2.0 * z + h[-1]) * h[-2] * m[..., -1]) / z
    s = np.linalg.solve(A, b.reshape(-1, n).T).T.reshape(y.shape)
    return _hermite(x, y, s, xq)
