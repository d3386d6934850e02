"""Generate tests/golden/gamma_grad_edges.npz: the implicit reparameterisation gradient of a standard-Gamma draw,

    d x / d a = -(d/da P(a, x)) / pdf(x; a),        P = the regularised lower incomplete gamma function,

with mpmath at 60 digits on the grid of tests/guide_edge_cases.gamma_grid (float64 points, and the same grid
rounded to float32 and evaluated at the rounded points).

    python tests/golden/make_golden_gamma_grad_edges.py

d/da P is mpmath.diff's central difference at h = 1e-20 (evaluated at twice the working precision) of
mpmath.gammainc(a, 0, x, regularized=True).  From a = 1e7 on gammainc gives up ("converges too slowly": its series
is capped at 6000 terms), and P is summed from the same series with the cap lifted:
P(a, x) = x^a e^-x / Gamma(a + 1) * 1F1(1; a + 1; x); the two agree to 1e-55 where both work (asserted below).
More than 14 standard deviations above the mean (points of the grid above a = 1e8 only) d/da P is taken as
-d/da Q, Q = 1 - P from Legendre's continued fraction: P itself is 1 to thousands of digits there.

<dtype>/a, <dtype>/x    the grid (float64 arrays; the float32 grid holds float32-representable values)
<dtype>/ref             the gradient, rounded to float64
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from tests import guide_edge_cases as gc  # noqa: E402

mp.mp.dps = 60
H = mp.mpf("1e-20")


def P_series(a, x):
    return mp.exp(a * mp.log(x) - x - mp.loggamma(a + 1)) * mp.hyp1f1(1, a + 1, x, maxterms=10 ** 8)


def P(a, x):
    try:
        return mp.gammainc(a, 0, x, regularized=True)
    except mp.libmp.NoConvergence:
        return P_series(a, x)


def Q_fraction(a, x):
    """The regularised UPPER function from Legendre's continued fraction (modified Lentz), for x > a."""
    tiny = mp.mpf("1e-500")
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 10 ** 7):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = 1 / (d if d != 0 else tiny)
        c = b + an / c
        c = c if c != 0 else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1) < mp.mpf(10) ** (-mp.mp.dps - 2):
            return mp.exp(a * mp.log(x) - x - mp.loggamma(a)) * h
    raise mp.libmp.NoConvergence("continued fraction of Q(%s, %s)" % (a, x))


def grad(a, x):
    a, x = mp.mpf(float(a)), mp.mpf(float(x))
    if x - a > 14 * mp.sqrt(a):
        # P = 1 - Q with Q below e^-98: the difference of two P would hold no digit of dP/da at any affordable
        # precision; d/da P = -d/da Q, and Q keeps its relative precision however small it is
        dP = -mp.diff(lambda t: Q_fraction(t, x), a, h=H)
    else:
        dP = mp.diff(lambda t: P(t, x), a, h=H)
    pdf = mp.exp((a - 1) * mp.log(x) - x - mp.loggamma(a))
    return float(-dP / pdf)


def main():
    for a, x in ((1e5, 1e5 + 3000.0), (1e5, 9.7e4), (30.0, 2.0)):
        a, x = mp.mpf(a), mp.mpf(x)
        assert abs(mp.gammainc(a, 0, x, regularized=True) - P_series(a, x)) < mp.mpf("1e-55")
    for a, x in ((1e5, 1e5 + 3000.0), (30.0, 45.0), (1e4, 1e4 + 1300.0)):
        a, x = mp.mpf(a), mp.mpf(x)
        q = mp.gammainc(a, x, mp.inf, regularized=True)
        assert abs(Q_fraction(a, x) - q) < mp.mpf("1e-50") * q
    flat = {}
    for f32 in (False, True):
        a, x = gc.gamma_grid(f32)
        ref = np.array([grad(ai, xi) for ai, xi in zip(a, x)])
        assert np.isfinite(ref).all()
        key = gc.dname(f32)
        flat[key + "/a"], flat[key + "/x"], flat[key + "/ref"] = a, x, ref
        print(key, a.size, "points; gradient in [%.3g, %.3g]" % (ref.min(), ref.max()))
    path = os.path.join(HERE, "gamma_grad_edges.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
