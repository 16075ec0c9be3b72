"""cultionet_amd.curves against scipy.interpolate (PchipInterpolator, CubicSpline with its default not-a-knot ends),
within 1e-12: both evaluate the same cubic pieces in float64, values here are of order 1-25, so 1e-12 leaves four
digits over the rounding of a handful of operations. Knot counts 3-7, T in {2, 5, 12, 25}, and the knots the draw of
cultionet_amd.augment uses: the warp knots for n in {1, 2}, the drift knots for m in 1..5 (m = 1 is the three-knot
spline, which scipy fits as one parabola)."""
import numpy as np
import pytest

from cultionet_amd import curves

TS = (2, 5, 12, 25)
BOUND = 1e-12


def _knots(g, n, T):
    x = np.sort(g.random(n)) * T
    x[0], x[-1] = 0.0, T
    assert (np.diff(x) > 0).all()
    return x


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7])
def test_random_knots_equal_scipy(n):
    si = pytest.importorskip("scipy.interpolate")
    g = np.random.default_rng(n)
    for T in TS:
        x, xq = _knots(g, n, T), np.arange(T, dtype=np.float64)
        walk = np.cumsum(g.normal(size=(4, 3, n)), axis=-1)   # both signs of slope: the flat-derivative rule of pchip
        rising = np.cumsum(g.random((5, n)), axis=-1)         # monotone, as the warp values are
        plateau = rising.copy()
        plateau[:, 1] = plateau[:, 2]                         # a zero secant slope
        for y in (walk, rising, plateau):
            assert np.abs(curves.pchip(x, y, xq) - si.PchipInterpolator(x, y, axis=-1)(xq)).max() <= BOUND
            assert np.abs(curves.cubic_spline(x, y, xq) - si.CubicSpline(x, y, axis=-1)(xq)).max() <= BOUND
        assert curves.pchip(x, walk, xq).shape == (4, 3, T) and curves.cubic_spline(x, rising, xq).shape == (5, T)


@pytest.mark.parametrize("n", [1, 2])
def test_warp_knots_equal_scipy(n):
    si = pytest.importorskip("scipy.interpolate")
    g = np.random.default_rng(10 + n)
    for T in TS:
        knots = np.concatenate(([0.0], (0.5 + np.arange(n)) / n * (T - 1), [T - 1.0]))
        values = np.concatenate((np.zeros((255, 1)), np.cumsum(g.random((255, n + 1)) + 0.1, axis=1)), axis=1)
        values = values / values[:, -1:] * (T - 1)
        xq = np.arange(T, dtype=np.float64)
        got = curves.pchip(knots, values, xq)
        assert np.abs(got - si.PchipInterpolator(knots, values, axis=1)(xq)).max() <= BOUND
        assert (np.diff(got, axis=1) >= 0).all() and np.abs(got[:, 0]).max() == 0 and np.abs(got[:, -1] - (T - 1)).max() <= BOUND


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_drift_knots_equal_scipy(m):
    si = pytest.importorskip("scipy.interpolate")
    g = np.random.default_rng(20 + m)
    for T in TS:
        knots = np.linspace(0.0, T, m + 2)
        anchors = np.cumsum(g.normal(size=(255, 3, m + 2)), axis=-1)
        xq = np.arange(T, dtype=np.float64)
        got = curves.cubic_spline(knots, anchors, xq)
        assert np.abs(got - si.CubicSpline(knots, anchors, axis=-1)(xq)).max() <= BOUND
        assert np.abs(got[..., 0] - anchors[..., 0]).max() <= BOUND


def test_without_scipy_the_curves_interpolate():
    """What holds whatever the derivative rule: the knots are met, two knots give the chord, three give the parabola."""
    x = np.array([0.0, 1.5, 4.0, 6.0])
    y = np.array([[1.0, -2.0, 0.5, 3.0], [0.0, 1.0, 2.0, 2.5]])
    for f in (curves.pchip, curves.cubic_spline):
        assert np.abs(f(x, y, x) - y).max() <= BOUND
        assert np.abs(f(x[:2], y[:, :2], np.array([0.75])) - y[:, :2].mean(axis=1, keepdims=True)).max() <= BOUND
    q = np.polyfit(x[:3], y[0, :3], 2)
    xq = np.linspace(0.0, 4.0, 9)
    assert np.abs(curves.cubic_spline(x[:3], y[0, :3], xq) - np.polyval(q, xq)).max() <= 1e-11
    for bad in (dict(x=x[::-1], y=y, xq=x), dict(x=x, y=y[:, :3], xq=x), dict(x=x, y=y, xq=np.array([7.0])),
                dict(x=x[:1], y=y[:, :1], xq=x[:1])):
        with pytest.raises(ValueError):
            curves.pchip(**bad)
