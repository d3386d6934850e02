"""Edge-of-range grids of the twelve site families, their float64 torch reference and the one
tolerance rule that test_dist_edges_host.py (the numpy oracle) and test_dist_edges_gpu.py (the HIP
kernels) share.

Reference: torch.distributions on the CPU with validate_args=False, gradients by autograd.  Binomial
(logits) and the two KL pieces are the formulas the kernels implement, written in torch.

Tolerance (one rule, every path):
  float64  the non-finite pattern (NaN, +inf, -inf) equals torch-f64's exactly; elsewhere
           |got - ref64| <= 64 eps64 M.
  float32  where torch's own f32 result is finite the kernel's is finite too, and
           |got - ref64| <= 4 |torch32 - ref64| + 8 eps32 M   (the "f32 class" rule);
           elements where torch-f32 is itself non-finite are not scored; a result below the f32
           normal range (2^-126) may be flushed to zero.
  M        the sum of the absolute values of the summands of the formula, in float64, a difference
           v - a counted as |v| + |a|, each log1p(exp(-|a|)) counted as 1 (the f32 path evaluates
           log2(1 + e) on purpose); lgamma(x) counts |lgamma x| + |(x - 1/2) ln x| + |x| (its Stirling
           summands), digamma(x) counts |ln(x + 6)| + sum_{k<6} 1/(x + k) (its six-step recurrence).
  A sum's M is the sum of its summands' M (times |scale|); a product with an exact power-of-two
  weight scales M by that weight.

Elements at which torch's own float64 result is wrong are listed in TORCH_DEFECTS and scored against
the exact value instead (see there).
"""
import math

import numpy as np
import torch

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
F32_TINY = float(np.finfo(np.float32).tiny)      # 2^-126
NAMES = {0: "Normal", 1: "Bernoulli", 2: "HalfCauchy", 3: "LogNormal", 4: "Exponential",
         5: "HalfNormal", 6: "Gamma", 7: "Beta", 8: "Poisson", 9: "Binomial", 10: "KLloc",
         11: "KLscale"}
TWO_PARAM = (0, 3, 6, 7, 9, 10)
INF, NAN = math.inf, math.nan
# the smallest normal f32 is 2^-126: scales below it are denormal in f32
F32_DENORMAL_SCALES = (2.0 ** -130, 1e-40, 2.0 ** -149)


def _prod(*lists):
    g = np.meshgrid(*[np.asarray(x, dtype=np.float64) for x in lists], indexing="ij")
    return [x.ravel() for x in g]


# one base point per family, each operand replaced in turn by NaN, +inf and -inf
_BASE = {0: (1.0, 0.5, 2.0), 1: (1.0, 0.3, 0.0), 2: (1.5, 2.0, 0.0), 3: (1.5, 0.2, 0.7),
         4: (1.5, 2.0, 0.0), 5: (1.5, 2.0, 0.0), 6: (1.5, 2.0, 3.0), 7: (0.3, 2.0, 3.0),
         8: (3.0, 2.5, 0.0), 9: (3.0, 0.3, 10.0), 10: (1.0, 0.5, 2.0), 11: (1.5, 2.0, 0.0)}


# and points where a NaN meets a zero coefficient: xlogy(0, NaN) is NaN
_EXTRA = {6: [(NAN, 1.0, 2.0)], 7: [(NAN, 1.0, 1.0), (NAN, 1.0, 3.0)]}


def _specials(dist_id):
    base = _BASE[dist_id]
    nops = 3 if dist_id in TWO_PARAM else 2
    pts = [list(p) for p in _EXTRA.get(dist_id, [])]
    for j in range(nops):
        for s in (NAN, INF, -INF):
            p = list(base)
            p[j] = s
            pts.append(p)
    return [np.array(c) for c in zip(*pts)]


def grid(dist_id, f32):
    """(v, a, b) float64 arrays of the family's edge grid (b = zeros for one-parameter families),
    already representable in the target precision."""
    scales = [1e-30, 1e-6, 1.0, 1e6, 1e30]
    if dist_id in (0, 10):
        z, loc, s = _prod([0.0, 0.75, -3.0, 1e15], [0.0, 2.5, -1e6], scales)
        v, a, b = loc + z * s, loc, s
    elif dist_id == 1:
        lg = [1e-8, 17.0, 40.0, 100.0, 1e30, INF]
        lg = lg + [-x for x in lg] + [0.0]
        v, a = _prod([0.0, 1.0], lg)
        b = np.zeros_like(v)
    elif dist_id == 2:
        s = [1e-20, 1e-10, 1.0, 1e10, 2e19, 3e19, 1e20]
        v, a = _prod([0.0, -0.0, -1.0, 1e-20, 1.0, 1e10, 1e19, 2e19, 3e19, 1e20, INF], s)
        b = np.zeros_like(v)
    elif dist_id == 3:
        tiny = 1e-37 if f32 else 1e-300
        v, a, b = _prod([tiny, 1e-6, 1.0, 2.5, 1e6, 1e30], [0.0, -5.0, 40.0], [1e-6, 1.0, 1e6])
    elif dist_id == 4:
        v, a = _prod([0.0, 1e-30, 1.0, 1e30], [1e-30, 1e-10, 1.0, 1e10, 1e30])
        b = np.zeros_like(v)
    elif dist_id == 5:
        v, a = _prod([0.0, -0.0, -1.0, 1e-30, 0.5, 3.0, 1e15, 1e30], scales)
        b = np.zeros_like(v)
    elif dist_id == 6:
        v, a, b = _prod([0.0, 1e-30, 1.0, 1e30], [1e-6, 1e-3, 1.4616321449683623, 1.0, 1e4, 1e7],
                        [1e-10, 1.0, 1e10])
    elif dist_id == 7:
        lo, hi = (2.0 ** -24, 1 - 2.0 ** -24) if f32 else (1e-300, 1 - 2.0 ** -53)
        v, a, b = _prod([0.0, lo, 0.5, hi, 1.0], [1e-3, 0.5, 1.0, 1e5], [1e-3, 1.0, 3.0, 1e5])
    elif dist_id == 8:
        v, a = _prod([0.0, 1.0, 1e6, 1e9], [0.0, 1e-30, 1.0, 1e6, 1e9])
        b = np.zeros_like(v)
    elif dist_id == 9:
        vs, as_, bs = [], [], []
        for n in (1.0, 10.0, 1e7):
            for k in (0.0, math.floor(n / 2), n):
                for lg in (50.0, -50.0, 1e30, -1e30, 0.3):
                    vs.append(k), as_.append(lg), bs.append(n)
        v, a, b = np.array(vs), np.array(as_), np.array(bs)
    elif dist_id == 11:
        v, a = _prod(scales, scales)
        b = np.zeros_like(v)
    sv, sa, sb = _specials(dist_id)
    v, a, b = np.concatenate([v, sv]), np.concatenate([a, sa]), np.concatenate([b, sb])
    if dist_id not in TWO_PARAM:
        b = np.zeros_like(v)
    if f32:
        with np.errstate(over="ignore"):
            v, a, b = (x.astype(np.float32).astype(np.float64) for x in (v, a, b))
    return v, a, b


def denormal_grid(dist_id):
    """f32 points whose scale operand is below 2^-126 (families whose kernel takes pos_log/pos_rcp
    of a scale): (v, a, b) float64 arrays exactly representable in f32."""
    s = np.array(F32_DENORMAL_SCALES).astype(np.float32).astype(np.float64)
    if dist_id in (0, 10):
        v, a, b = s * 0.5, np.zeros_like(s), s
    elif dist_id == 11:
        v, a, b = s, s * 4, np.zeros_like(s)           # sq denormal and sp denormal
        v = np.concatenate([v, np.ones_like(s)])
        a = np.concatenate([np.ones_like(s), s])
        b = np.zeros_like(v)
    else:
        raise ValueError(dist_id)
    return v, a, b


# ---- the torch reference -----------------------------------------------------------------------

def torch_log_prob(dist_id, v, a, b):
    D = torch.distributions
    if dist_id == 0:
        return D.Normal(a, b, validate_args=False).log_prob(v)
    if dist_id == 1:
        return D.Bernoulli(logits=a, validate_args=False).log_prob(v)
    if dist_id == 2:
        return D.HalfCauchy(a, validate_args=False).log_prob(v)
    if dist_id == 3:
        return D.LogNormal(a, b, validate_args=False).log_prob(v)
    if dist_id == 4:
        return D.Exponential(a, validate_args=False).log_prob(v)
    if dist_id == 5:
        return D.HalfNormal(a, validate_args=False).log_prob(v)
    if dist_id == 6:
        return D.Gamma(a, b, validate_args=False).log_prob(v)
    if dist_id == 7:
        return D.Beta(a, b, validate_args=False).log_prob(v)
    if dist_id == 8:
        return D.Poisson(a, validate_args=False).log_prob(v)
    if dist_id == 9:      # k*logit - n*softplus(logit) + log C(n, k)
        sp = a.clamp(min=0) + torch.log1p(torch.exp(-a.abs()))
        return v * a - b * sp + torch.lgamma(b + 1) - torch.lgamma(v + 1) - torch.lgamma(b - v + 1)
    if dist_id == 10:     # -KL(N(lq, sq) || N(lp, sp)) = this(lq; lp, sp) + piece 11(sq; sp)
        return -0.5 * ((v - a) / b) ** 2 - torch.log(b)
    if dist_id == 11:
        return torch.log(v) + 0.5 - 0.5 * (v / a) ** 2
    raise ValueError(dist_id)


# Elements where torch's float64 result is not the value of the formula: (dist_id, output, predicate
# on (v, a, b), the exact value used instead).
#  - Bernoulli: torch evaluates -BCEWithLogits as (1 - v) * logits - logsigmoid(logits), so value 1
#    at logits -inf gives 0 * (-inf) = NaN; the density is 0 there, its log -inf.
#  - d/dscale at an infinite scale, value and loc finite: autograd through scale**2 multiplies 0 by
#    inf (NaN); the derivative of the formula, -1/s + d^2/s^3, is 0 there.
#  - Binomial d/dlogits at an infinite total_count: the clamp + log1p split of softplus gives
#    -inf + inf; the derivative of the formula is k - n * sigmoid(logits).
def _inf_scale(s, *finite):
    return np.isinf(s) & np.logical_and.reduce([np.isfinite(x) for x in finite])


TORCH_DEFECTS = [
    (1, "lp", lambda v, a, b: (v == 1) & (a == -INF), -INF),
    (0, "db", lambda v, a, b: _inf_scale(b, v, a), 0.0),
    (3, "db", lambda v, a, b: _inf_scale(b, v, a) & (v > 0), 0.0),
    (5, "da", lambda v, a, b: _inf_scale(a, v) & (v >= 0), 0.0),
    (10, "db", lambda v, a, b: _inf_scale(b, v, a), 0.0),
    (9, "da", lambda v, a, b: _inf_scale(b, v, a), lambda v, a, b: v - b / (1 + np.exp(-a))),
]
# Elements where the kernels keep a NaN that torch does not have, left as they are because the fix
# would change an arithmetic path the benchmark runs: (dist_id, output, predicate).
#  - Bernoulli at value 0, logits +inf: v * logits - softplus(logits) is 0 * inf; torch gives -inf.
KEPT_NAN = [
    (1, "lp", lambda v, a, b: (v == 0) & (a == INF)),
]


def kept_nan(dist_id, what, v, a, b):
    """bool mask of the elements where a NaN is accepted in place of the reference (KEPT_NAN)."""
    m = np.zeros(np.shape(v), dtype=bool)
    for did, w, pred in KEPT_NAN:
        if did == dist_id and w == what:
            m |= pred(v, a, b)
    return m


def reference(dist_id, v, a, b, dtype=torch.float64):
    """dict lp, dv, da, db (numpy float64) of torch evaluated in ``dtype`` at the given points."""
    ts = [torch.tensor(x, dtype=dtype).requires_grad_(True) for x in (v, a, b)]
    lp = torch_log_prob(dist_id, *ts)
    gs = torch.autograd.grad(lp.sum(), ts, allow_unused=True)
    out = {"lp": lp.detach()}
    for k, g in zip(("dv", "da", "db"), gs):
        out[k] = torch.zeros_like(ts[0]) if g is None else g
    out = {k: x.double().numpy() for k, x in out.items()}
    if dtype == torch.float64:
        for did, what, pred, val in TORCH_DEFECTS:
            if did == dist_id:
                with np.errstate(all="ignore"):
                    val = val(v, a, b) if callable(val) else val
                out[what] = np.where(pred(v, a, b), val, out[what])
    return out


# ---- magnitudes M --------------------------------------------------------------------------------

def _lgM(x):
    from scipy.special import gammaln
    return np.abs(gammaln(x)) + np.abs((x - 0.5) * np.log(np.abs(x))) + np.abs(x)


def _psiM(x):
    return np.abs(np.log(x + 6)) + sum(1 / np.abs(x + k) for k in range(6))


def _xlm(x, y):
    """magnitude of xlogy(x, y): 0 where x == 0."""
    return np.where(x == 0, 0.0, np.abs(x) * np.abs(np.log(np.abs(y))))


def magnitude(dist_id, v, a, b):
    """dict lp, dv, da, db of M (float64) at the points."""
    with np.errstate(all="ignore"):
        c = 0.5 * math.log(2 * math.pi)
        if dist_id in (0, 10, 5, 3):
            if dist_id == 5:
                v, a, b = v, np.zeros_like(v), a
            L = np.abs(np.log(v)) if dist_id == 3 else 0.0
            x = np.log(v) if dist_id == 3 else v
            u = np.abs(x) + np.abs(a)
            lp = u * u / (2 * b * b) + np.abs(np.log(b)) + (0.0 if dist_id == 10 else c) + L
            dloc = u / (b * b)
            dsc = u * u / np.abs(b) ** 3 + 1 / np.abs(b)
            dv = (dloc + 1) / np.abs(v) if dist_id == 3 else dloc
            if dist_id == 5:
                return {"lp": lp + math.log(2), "dv": dv, "da": dsc, "db": 0 * v}
            return {"lp": lp, "dv": dv, "da": dloc, "db": dsc}
        if dist_id == 1:
            return {"lp": np.abs(v * a) + np.maximum(a, 0) + 1, "dv": np.abs(a),
                    "da": np.abs(v) + 1, "db": 0 * v}
        if dist_id == 2:
            q = v / a
            return {"lp": 0.46 + np.abs(np.log(a)) + np.log1p(q * q),
                    "dv": 2 * np.abs(q) / (np.abs(a) * (1 + q * q)), "da": 1 / np.abs(a), "db": 0 * v}
        if dist_id == 4:
            return {"lp": np.abs(np.log(a)) + np.abs(a * v), "dv": np.abs(a),
                    "da": 1 / np.abs(a) + np.abs(v), "db": 0 * v}
        if dist_id == 11:
            return {"lp": np.abs(np.log(v)) + 0.5 + v * v / (2 * a * a),
                    "dv": 1 / np.abs(v) + np.abs(v) / (a * a), "da": v * v / np.abs(a) ** 3, "db": 0 * v}
        am1 = np.where(a == 1, 0.0, np.abs(a) + 1)
        if dist_id == 6:
            return {"lp": _xlm(a, b) + _xlm(am1, v) + np.abs(b * v) + _lgM(a),
                    "dv": am1 / np.abs(v) + np.abs(b),
                    "da": _xlm(a != 0, b) + _xlm(a != 1, v) + _psiM(a),
                    "db": np.abs(a / b) + np.abs(v)}
        if dist_id == 7:
            bm1 = np.where(b == 1, 0.0, np.abs(b) + 1)
            u = 1 - v
            return {"lp": _xlm(am1, v) + _xlm(bm1, u) + _lgM(a + b) + _lgM(a) + _lgM(b),
                    "dv": am1 / np.abs(v) + bm1 / np.abs(u),
                    "da": _xlm(a != 1, v) + _psiM(a + b) + _psiM(a),
                    "db": _xlm(b != 1, u) + _psiM(a + b) + _psiM(b)}
        if dist_id == 8:
            return {"lp": _xlm(v, a) + np.abs(a) + _lgM(v + 1),
                    "dv": _xlm(v != 0, a) + _psiM(v + 1),
                    "da": np.abs(v / a) + 1, "db": 0 * v}
        if dist_id == 9:
            sp = np.maximum(a, 0) + 1
            return {"lp": np.abs(v * a) + np.abs(b) * sp + _lgM(b + 1) + _lgM(v + 1) + _lgM(b - v + 1),
                    "da": np.abs(v) + np.abs(b),
                    "dv": np.abs(a) + _psiM(v + 1) + _psiM(b - v + 1),
                    "db": _psiM(b + 1) + _psiM(b - v + 1) + sp}
    raise ValueError(dist_id)


# ---- the rule ----------------------------------------------------------------------------------------

def _fmt(idx, inputs, got, ref, bound):
    lines = []
    for i in idx[:8]:
        pt = ", ".join("%.17g" % x[i] for x in inputs)
        lines.append("  at (%s): got %.17g ref %.17g bound %.3g" % (pt, got[i], ref[i], bound[i]
                                                                    if np.ndim(bound) else bound))
    return "\n".join(lines)


def check(what, got, ref64, M, f32, ref32=None, inputs=(), nan_ok=None):
    """Assert the module's tolerance rule; ``inputs`` (arrays of the same shape) only label failures,
    ``nan_ok`` marks elements where a NaN is accepted (KEPT_NAN)."""
    got = np.asarray(got, dtype=np.float64)
    shape = got.shape
    inputs = [np.broadcast_to(np.asarray(x, dtype=np.float64), shape).ravel() for x in inputs]
    got = got.ravel()
    if nan_ok is not None:
        nan_ok = np.broadcast_to(nan_ok, shape).ravel()
        got = got.copy()
        got[nan_ok & np.isnan(got)] = np.broadcast_to(np.asarray(ref64, dtype=np.float64),
                                                      shape).ravel()[nan_ok & np.isnan(got)]
    ref64 = np.broadcast_to(np.asarray(ref64, dtype=np.float64), shape).ravel()
    M = np.broadcast_to(np.asarray(M, dtype=np.float64), shape).ravel()
    with np.errstate(all="ignore"):
        if not f32:
            bad = ((np.isnan(got) != np.isnan(ref64)) | ((got == INF) != (ref64 == INF)) |
                   ((got == -INF) != (ref64 == -INF)))
            fin = np.isfinite(ref64) & np.isfinite(got)
            bound = 64 * EPS64 * M
            bad |= fin & ~(np.abs(got - ref64) <= bound)
        else:
            ref32 = np.broadcast_to(np.asarray(ref32, dtype=np.float64), shape).ravel()
            scored = np.isfinite(ref32)
            bound = 4 * np.abs(ref32 - ref64) + 8 * EPS32 * M + F32_TINY
            err = np.where(got == ref64, 0.0, np.abs(got - ref64))
            bad = scored & (~np.isfinite(got) | ~(err <= bound))
    idx = np.flatnonzero(bad)
    assert idx.size == 0, "%s: %d of %d elements out of tolerance\n%s" % (
        what, idx.size, got.size, _fmt(idx, inputs, got, ref64, np.broadcast_to(bound, got.shape)))
