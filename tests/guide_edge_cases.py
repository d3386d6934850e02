"""Case grids, references and the tolerance rule of the kernels that end every SVI step: the flat Adam /
ClippedAdam update (csrc/optim.hip, csrc/optim_dev.h), the reparameterised Gamma draw with its implicit
gradient (csrc/gamma.hip), the full-covariance guide's draw and backward (csrc/mvn_guide.hip) and the two
site kernels of csrc/guide_site.hip.  test_guide_edges_host.py runs the numpy oracles (oracle/adam.py,
oracle/gamma.py, tests/oracle_backend.py) against these references on the CPU, test_guide_edges_gpu.py the
HIP kernels.

References (float64, independent of the kernels and of oracle/):
  Adam         torch.optim.Adam(foreach=False) on float64 CPU tensors, one step from a preset state (the
               moments and ``state["step"]`` are written into the optimizer's state), moments read back.
  ClippedAdam  the unmodified reference's pyro.optim.clipped_adam.ClippedAdam, recorded by
               tests/golden/make_golden_adam_edges.py into tests/golden/adam_edges.npz on a pool of
               ADAM_POOL = 61 elements per case.  The update is element-wise, so a case of n elements reads
               the pool cyclically (element i = pool element i mod 61; 61 is prime to the 64 lanes and the
               256 threads, so a misplaced element differs from its neighbour in every launch geometry).
               ``group["lr"]`` is preset to lr * lrd**step0: the reference multiplies it by lrd once per step.
               An lrd < 1 is not combined with step0 = 100 000: lr * 0.99**100001 underflows to 0, which the
               kernel documents as the no-op optimizer (moments stay) while the reference still moves them.
               The edge gradient 1e25 is recorded too: ClippedAdam clamps it to clip_norm before anything
               overflows, plain Adam squares it (float32: exp_avg_sq = inf, as the CPU formula gives).
  Gamma grad   -(d/da P(a, x)) / pdf(x; a), P = the regularised lower incomplete gamma function, by a central
               difference (h = 1e-20) at 60 digits with mpmath: tests/golden/gamma_grad_edges.npz, written by
               tests/golden/make_golden_gamma_grad_edges.py.  The float32 points are stored at their
               float32-rounded (a, x).
  Gamma draws  oracle.gamma.standard_gamma (the same Philox blocks) at the project's 1e-12 / 5e-7, and the
               Kolmogorov-Smirnov distance to scipy.stats.gamma.
  mvn forward  z = loc + eps @ T^T, T = softplus(rho)[:, None] * (tril(A, -1) + I); log q from
               torch.distributions.MultivariateNormal(0, scale_tril=T).log_prob(eps @ T^T): the centred form of
               the existing test's reference.  (log_prob(z) of the un-centred distribution first forms z - loc:
               with rho = -30 beside loc = O(1), or loc = 1e4 beside scales of 1e-3, that difference has lost
               3 to 9 of its 16 digits before the triangular solve sees it -- an error of the reference, not of
               the kernel, which never forms the difference in the forward pass.)
  mvn backward autograd of sum(d_z z) + sum(d_logq log q) with log q = -|eps|^2/2 - sum log S - n/2 log 2 pi.
               The triangular-solve form of log q is the same function of (loc, rho, A), but its autograd
               cancels terms of size 1/S_k: with one rho = -30 the residue is ~1e-3, above every bound here.
               The host test pins the two forms on each other where every rho is ordinary.
  exp site     float64 torch: value = lower + exp(u), log_density = -sum_event u, d u = g_value (value - lower)
               - g_ld.
  score        float64 torch Normal(loc, scale).log_prob(z).sum() * coef; gradient -coef P / scale.

Tolerance: the "f32 class" rule of tests/enum_edge_cases.py / tests/dist_edge_cases.py (``check`` is imported
from there):
  float64  the non-finite pattern equals the reference's exactly; elsewhere |got - ref64| <= 64 eps64 M.
  float32  |got - ref64| <= 4 |cpu32 - ref64| + 8 eps32 M, cpu32 = the same plain torch formula in float32 on
           the CPU; elements where cpu32 is non-finite while ref64 is finite are not scored (at most 5 % of a
           case, asserted).
  M, the magnitude of what was summed, per output:
    Adam  g' = clamp(g) + wd p has magnitude G = |clamp(g)| + wd |p|
          exp_avg      |m| + G
          exp_avg_sq   |v| + G^2
          parameter    |p| + step_size (|m| + G) / denom: the update with the moment replaced by the magnitude
                       of its two terms (>= |update|; the moment may cancel, and the parameter inherits the
                       moment's absolute error divided by denom)
    mvn   z_i          |loc_i| + S_i (sum_{j<i} |A_ij eps_j| + |eps_i|)
          log q        sum eps^2 / 2 + sum |log S_i| + n/2 log 2 pi
          d_loc_i      sum_p |d_z[p, i]|
          d_A_ij       S_i sum_p |d_z[p, i] eps[p, j]| below the diagonal; exactly 0 on and above it
          d_rho_i      sigmoid(rho_i) (sum_p |d_z[p, i]| (|z[p, i]| + |loc_i|) / S_i + sum_p |d_logq[p]| / S_i):
                       the backward recovers u = (z - loc) / S from z, so |z| + |loc| is what it sums
    site  value        |lower| + exp(u);  log_density: sum |u| over the row
          d u          |g_value| (|value| + |lower|) + |g_ld|
          score        |coef| (sum e^2 / 2 + P sum |log scale| + P n log sqrt(2 pi)); gradient |coef| P / scale
  Gamma gradient (not a sum): relative, per branch.  The host test measures oracle.gamma.implicit_grad against
  the fixture; the device bound is 4 x that maximum (GAMMA_HOST_MAX below), never above 1e-9; float32 adds
  2^-23 |ref| (the float64 evaluation rounded once).  One departure from a purely relative bound: the dtype's
  smallest normal (2^-1022, in float32 2^-126) is added, because results below it may be flushed to zero; the
  fixture's smallest references are 5.4e-314 and 4.2e-45.

  The branch that used to serve the tails of a > 1e8 (the normal limit 1 + (x - a) / 2a) was 2.4e-7 off at 12
  standard deviations beside a = 1e8 -- a jump of that size at the seam -- and returned 0.5 at the clamp values
  (reference 1.6e-313): csrc/gamma.hip and oracle/gamma.py now take the Cornish-Fisher form within a / 100 of the
  mean there and the series / continued fraction beyond.  The grid holds, above a = 1e8, points at 50 standard
  deviations, at a (1 -+ 0.005), either side of a (1 -+ 0.01) and at a (1 -+ 0.05), a (1 -+ 0.09), a (1 -+ 0.3).
  Against the fixture the form is 2.7e-12 off at 0.05, 1.0e-10 at 0.09 and 3.2e-7 at 0.3 (a = 3e8, CPU), the series
  and the continued fraction below 1e-13 at all three: a seam moved out to a / 10 misses the bound of 1.1e-11 at
  0.09, a condition with the wrong sign misses it at twelve points.

Measured maxima of the gradient over the fixture, |got - ref| / |ref| per branch (references below 1e-290, in
float32 1e-30, left out: they hold few digits):
                    host oracle (CPU)    device f64 (MI355X)    device f32 (MI355X)    device bound f64
  series            2.72e-12             2.72e-12               4.88e-08               1.12e-11
  fraction          2.94e-12             2.93e-12               5.47e-08               1.20e-11
  cornish           3.45e-11             3.45e-11               5.81e-08               1.40e-10
(the kernel header's 4e-11 for the Cornish-Fisher form at a = 1e4 holds: the maximum sits at a = 1e4, x = 9201).
Kolmogorov-Smirnov p-values of the 50 000 float64 draws at seed 42, offset 1000, device = host oracle to the
digits shown: a = 0.05: 0.80, 0.5: 0.22, 0.999: 0.52, 1: 0.44, 1.001: 0.44, 30: 0.45, 1e3: 0.48, 1e5: 0.49.

Largest error / bound per kernel, path and dtype, measured on the MI355X by test_guide_edges_gpu.py (every case
of the module; 1.0 would be the bound).  Every float32 Adam case also ran as a lone phase of a recorded chain
(one chain kernel, one phase: rec.stats == (1, 1)), bit-equal to the standalone launch.
  adam/edge/f32                0.250        clipped/edge/f32             0.057
  adam/edge/f64                0.012        clipped/edge/f64             0.012
  adam/lr0wd/f32               0.047        clipped/lr0wd/f32            0.047
  adam/lr0wd/f64               0.008        clipped/lr0wd/f64            0.011
  adam/one_wg/f32              0.047        clipped/one_wg/f32           0.047
  adam/one_wg/f64              0.054        clipped/one_wg/f64           0.050
  adam/single/f32              0.067        clipped/single/f32           0.067
  adam/single/f64              0.054        clipped/single/f64           0.050
  adam/stride/f32              0.047        clipped/stride/f32           0.047
  adam/stride/f64              0.054        clipped/stride/f64           0.050
  adam/ticket/f32              0.047        clipped/ticket/f32           0.047
  adam/ticket/f64              0.012        clipped/ticket/f64           0.012
  adam/traj/f64                0.018        clipped/traj/f64             0.010
  gamma/grad/cornish/f32       0.487        gamma/grad/cornish/f64       0.246
  gamma/grad/fraction/f32      0.459        gamma/grad/fraction/f64      0.245
  gamma/grad/series/f32        0.409        gamma/grad/series/f64        0.243
  mvn/row_per_thread/f32       0.205        mvn/row_per_thread/f32/sinks 0.176
  mvn/row_per_thread/f64       0.072        mvn/row_per_thread/f64/sinks 0.034
  mvn/wave_per_row/f32         0.362        mvn/wave_per_row/f32/sinks   0.161
  mvn/wave_per_row/f64         0.142        mvn/wave_per_row/f64/sinks   0.030
  score/blocks/f32             0.048        score/blocks/f64             0.015
  score/capped/f32             0.050        score/capped/f64             0.008
  site/loop/f32                0.121        site/loop/f64                0.029
  site/rows/f32                0.075        site/rows/f64                0.019
  (value-only launches of the site kernel: 0.121 / 0.029 looping, 0.069 / 0.019 otherwise)
"""
import functools
import math
import os

import numpy as np
import torch

from tests.enum_edge_cases import (EPS32, EPS64, F32, F32_TINY, F64, INF, NAN, RATIOS, UNSCORED_CAP, check,  # noqa: F401
                                   unscored_fraction)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LABEL_PREFIXES = ("adam/", "clipped/", "gamma/", "mvn/", "site/", "score/")


def ratio_table():
    return "\n".join("  %-28s %.3f" % (k, v) for k, v in sorted(RATIOS.items()) if k.startswith(LABEL_PREFIXES))


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def kind(x):
    x = np.asarray(x, np.float64)
    return np.isnan(x) * 1 + (x == INF) * 2 + (x == -INF) * 3


def to32(x):
    """float64 values that float32 holds exactly."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def dt(f32):
    return F32 if f32 else F64


def dname(f32):
    return "f32" if f32 else "f64"


# =======================================================================================================
# Adam / ClippedAdam
# =======================================================================================================
ADAM_LR = 0.01
ADAM_BETAS = ((0.9, 0.999), (0.0, 0.5), (0.95, 0.95))
ADAM_EPS = (1e-8, 1e-3)
ADAM_WD = (0.0, 0.1)
ADAM_CLIP = (10.0, 0.5)
ADAM_LRD = (1.0, 0.99)
ADAM_STEP0 = (0, 1, 999, 100000)
ADAM_N = (1, 2, 255, 256, 257, 1000)
ADAM_POOL = 61
ADAM_BIG_AT = (20, 40, 55)          # pool elements with g = 1e25: 12 of n = 257, under the 5 % cap
ADAM_NAN_AT, ADAM_INF_AT = 3, 7
ADAM_TRAJ_STEPS = 5


def adam_grid_stride_n(cus):
    """One n past the launch's cap of 8 * CUs workgroups of 256: threads loop."""
    return 8 * cus * 256 + 257


def adam_hypers(clipped):
    """Every hyper-parameter set of the issue's cross; index 0 is the default set."""
    out = []
    for betas in ADAM_BETAS:
        for eps in ADAM_EPS:
            for wd in ADAM_WD:
                for clip in (ADAM_CLIP if clipped else (0.0,)):
                    for lrd in (ADAM_LRD if clipped else (1.0,)):
                        out.append({"lr": ADAM_LR, "betas": betas, "eps": eps, "wd": wd, "clip": clip, "lrd": lrd})
    return out


ADAM_TRAJ_HYPER = {"lr": ADAM_LR, "betas": (0.9, 0.999), "eps": 1e-8, "wd": 0.1, "clip": 0.5, "lrd": 0.99}
ADAM_LR0WD_HYPER = {"lr": 0.0, "betas": (0.9, 0.999), "eps": 1e-8, "wd": 0.1, "clip": 10.0, "lrd": 1.0}


def adam_step0_of(clipped, h):
    """The preset step count of hyper-parameter set h: cycles so that every count meets every beta pair,
    eps and weight decay."""
    s = ADAM_STEP0[(h + h // 4) % 4]
    if adam_hypers(clipped)[h]["lrd"] != 1.0 and s == 100000:
        s = 999                                    # (lr * lrd**100001 = 0: see the docstring)
    return s


def adam_single_keys(clipped):
    """[(h, step0)] of the single-step cases: the default set at every preset count, every other set at one."""
    return [(0, s) for s in ADAM_STEP0] + [(h, adam_step0_of(clipped, h)) for h in range(1, len(adam_hypers(clipped)))]


def adam_pool():
    return {k: golden("adam_edges")["pool/" + k] for k in "pgmv"}


def make_adam_pool():
    """The generator's pool (float32-representable): p, m of order 1, v > 0, and g = 0.74 N(0, 1), which the
    clamp at 0.5 touches on about half the elements."""
    r = np.random.default_rng(20240607)
    n = ADAM_POOL
    return {"p": to32(r.standard_normal(n)), "g": to32(0.74 * r.standard_normal(n)),
            "m": to32(0.5 * r.standard_normal(n)), "v": to32((0.6 * r.standard_normal(n)) ** 2 + 1e-3)}


def adam_inputs(pool, hy, n, variant=None):
    """(p, g, m, v) float64, float32-representable, n elements read cyclically from the pool.  With eps = 1e-3
    the gradient and the first moment are of order 1e-3 and the second of order 1e-6: eps decides the result."""
    s = 1e-3 if hy["eps"] == 1e-3 else 1.0
    p, g, m, v = pool["p"].copy(), to32(pool["g"] * s), to32(pool["m"] * s), to32(pool["v"] * s * s)
    if variant == "zero":
        g, m, v = np.zeros_like(g), np.zeros_like(m), np.zeros_like(v)
    elif variant == "zero_state":
        g = np.zeros_like(g)
    elif variant == "naninf":
        g[ADAM_NAN_AT], g[ADAM_INF_AT] = NAN, INF
    elif variant == "big":
        g[list(ADAM_BIG_AT)] = to32(1e25)
    elif variant is not None:
        raise ValueError(variant)
    return tuple(np.resize(x, n) for x in (p, g, m, v))


def adam_traj_grad(pool, s):
    return to32(np.roll(pool["g"], 7 * s) * (1.0 + 0.25 * s))


def torch_adam_step(p, g, m, v, step0, hy, dtype):
    """One step of torch.optim.Adam (single-tensor path) from the given state -> (p, m, v) float64 numpy."""
    P = torch.tensor(p, dtype=dtype, requires_grad=True)
    P.grad = torch.tensor(g, dtype=dtype)
    opt = torch.optim.Adam([P], lr=hy["lr"], betas=hy["betas"], eps=hy["eps"], weight_decay=hy["wd"],
                           foreach=False)
    opt.state[P] = {"step": torch.tensor(float(step0)), "exp_avg": torch.tensor(m, dtype=dtype),
                    "exp_avg_sq": torch.tensor(v, dtype=dtype)}
    opt.step()
    st = opt.state[P]
    assert float(st["step"]) == step0 + 1
    return tuple(x.detach().double().numpy() for x in (P, st["exp_avg"], st["exp_avg_sq"]))


def torch_clipped_adam_step(p, g, m, v, step0, hy, dtype):
    """ClippedAdam's update as plain torch operators in ``dtype`` (the float32 comparison of the rule; the
    host test pins it to the recorded reference in float64)."""
    p, g, m, v = (torch.tensor(x, dtype=dtype) for x in (p, g, m, v))
    b1, b2 = hy["betas"]
    step = step0 + 1
    g = g.clamp(-hy["clip"], hy["clip"])
    if hy["wd"] != 0:
        g = g.add(p, alpha=hy["wd"])
    m = m.mul(b1).add(g, alpha=1 - b1)
    v = v.mul(b2).addcmul(g, g, value=1 - b2)
    denom = v.sqrt().add(hy["eps"])
    step_size = hy["lr"] * hy["lrd"] ** step * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    p = p.addcdiv(m, denom, value=-step_size)
    return tuple(x.double().numpy() for x in (p, m, v))


def adam_magnitudes(p, g, m, v, step0, hy, clipped, v_new):
    """(M_p, M_m, M_v) of the docstring."""
    b1, b2 = hy["betas"]
    step = step0 + 1
    with np.errstate(all="ignore"):
        gc = np.clip(g, -hy["clip"], hy["clip"]) if clipped and hy["clip"] > 0 else g
        G = np.abs(gc) + hy["wd"] * np.abs(p)
        Mm = np.abs(m) + G
        Mv = np.abs(v) + G * G
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        if clipped:
            upd = hy["lr"] * hy["lrd"] ** step * math.sqrt(bc2) / bc1 * Mm / (np.sqrt(v_new) + hy["eps"])
        else:
            upd = hy["lr"] / bc1 * Mm / (np.sqrt(v_new) / math.sqrt(bc2) + hy["eps"])
        Mp = np.abs(p) + upd
    return tuple(np.nan_to_num(x, nan=0.0, posinf=0.0) for x in (Mp, Mm, Mv))


def adam_golden_key(h, step0, variant=None):
    return "C/v_%s" % variant if variant else "C/h%d_s%d" % (h, step0)


def adam_hyper_of(clipped, h, variant=None):
    if variant == "lr0wd":
        return ADAM_LR0WD_HYPER
    return adam_hypers(clipped)[h]


@functools.lru_cache(maxsize=None)
def adam_case(clipped, h, step0, n, f32, variant=None):
    """dict: p, g, m, v (float64 inputs), hy, step0, ref = (p, m, v) float64, cpu32 (f32 cases), M = (Mp, Mm, Mv).
    ``variant`` "lr0wd": lr = 0 with weight decay (the moments move)."""
    hy = adam_hyper_of(clipped, h, variant)
    pool = adam_pool()
    inp = adam_inputs(pool, hy, n, None if variant == "lr0wd" else variant)
    with np.errstate(all="ignore"):
        if clipped:
            key = adam_golden_key(h, step0, variant)
            ref = tuple(np.resize(golden("adam_edges")[key + "/" + w], n) for w in "pmv")
        else:
            ref = torch_adam_step(*inp, step0, hy, F64)
        cpu32 = None
        if f32:
            cpu32 = (torch_clipped_adam_step if clipped else torch_adam_step)(*inp, step0, hy, F32)
        M = adam_magnitudes(*inp, step0, hy, clipped, ref[2])
    return {"p": inp[0], "g": inp[1], "m": inp[2], "v": inp[3], "hy": hy, "step0": step0, "ref": ref,
            "cpu32": cpu32, "M": M, "clipped": clipped}


def adam_check(label, got, case, f32):
    """The rule on (parameter, exp_avg, exp_avg_sq); in float32 the non-finite pattern is the CPU formula's."""
    c32 = case["cpu32"] or (None, None, None)
    for what, g, r, M, c in zip(("param", "exp_avg", "exp_avg_sq"), got, case["ref"], case["M"], c32):
        check(label, what, g, r, M, f32, c)
        if f32:
            assert (kind(g) == kind(c)).all(), "%s %s: non-finite pattern differs from the float32 CPU formula" % (
                label, what)


@functools.lru_cache(maxsize=None)
def adam_trajectory(clipped):
    """Five steps from zero moments in float64: (p0, [g_s], [(p, m, v) after step s])."""
    pool = adam_pool()
    grads = [adam_traj_grad(pool, s) for s in range(ADAM_TRAJ_STEPS)]
    if clipped:
        z = golden("adam_edges")
        return pool["p"], grads, [tuple(z["C/traj/" + w][s] for w in "pmv") for s in range(ADAM_TRAJ_STEPS)]
    hy = ADAM_TRAJ_HYPER
    P = torch.tensor(pool["p"], dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([P], lr=hy["lr"], betas=hy["betas"], eps=hy["eps"], weight_decay=hy["wd"], foreach=False)
    out = []
    for g in grads:
        P.grad = torch.tensor(g, dtype=F64)
        opt.step()
        st = opt.state[P]
        out.append(tuple(x.detach().clone().numpy() for x in (P, st["exp_avg"], st["exp_avg_sq"])))
    return pool["p"], grads, out


# =======================================================================================================
# Gamma: the implicit gradient and the draws
# =======================================================================================================
GAMMA_A = (1e-3, 1e-2, 0.05, 0.3, 0.999, 1.0, 1.001, 3.0, 30.0, 300.0, 1000.0, 3000.0, 9999.0, 1e4 * (1 - 1e-12), 1e4,
           1e5, 1e7, 1e8, float(np.nextafter(1e8, INF)), 3e8)
GAMMA_Q_LOWER = (1e-30, 1e-12, 1e-6, 1e-3, 0.1, 0.5)         # P(a, x) = q
GAMMA_Q_UPPER = (0.1, 1e-3, 1e-6, 1e-12)                     # 1 - P(a, x) = q
GAMMA_SIGMAS = (7.99, 8.01, 12.0)
GAMMA_WIDE_REL = (0.005, 0.00999, 0.01001, 0.05, 0.09, 0.3)       # |x - a| / a above a = 1e8: the seam is at 0.01
GAMMA_BRANCHES = ("series", "fraction", "cornish")
GAMMA_DEVICE_CAP = 1e-9
# |oracle.gamma.implicit_grad - fixture| / |fixture|, largest per branch over both grids (measured on the CPU by
# test_guide_edges_host.py, which asserts that the figures still hold)
GAMMA_HOST_MAX = {"series": 2.8e-12, "fraction": 3.0e-12, "cornish": 3.5e-11}
GAMMA_KS_A = (0.05, 0.5, 0.999, 1.0, 1.001, 30.0, 1e3, 1e5)
GAMMA_KS_N, GAMMA_KS_SEED, GAMMA_KS_OFFSET, GAMMA_KS_P = 50000, 42, 1000, 1e-3


def gamma_grid(f32, with_quantile_mask=False):
    """(a, x) float64 arrays of the gradient's grid, exactly representable in the target precision: per
    concentration the ten quantiles, x = a + 1 and the float below it, from a = 1e4 on a -+ 7.99, 8.01 and 12
    standard deviations, above a = 1e8 a -+ 50 standard deviations and a (1 -+ r) for the r of GAMMA_WIDE_REL
    (inside the Cornish-Fisher form's a / 100, either side of that seam, and far out where only the series and
    the continued fraction are right), and the clamp values 2^-126 (and 2^-1022 in float64).  Points whose x is
    below the dtype's smallest normal collapse onto the clamp value.  ``with_quantile_mask``: also True where x
    came from scipy's inverse (everything else is arithmetic on a)."""
    from scipy.special import gammainccinv, gammaincinv
    ft = np.float32 if f32 else np.float64
    tiny = float(np.finfo(ft).tiny)
    pts = []
    for a in GAMMA_A:
        a = float(ft(a))
        xs = [float(gammaincinv(a, q)) for q in GAMMA_Q_LOWER] + [float(gammainccinv(a, q)) for q in GAMMA_Q_UPPER]
        nq = len(xs)
        seam = ft(a) + ft(1)
        xs += [float(seam), float(np.nextafter(seam, ft(0)))]
        if a >= float(ft(1e4 * (1 - 1e-12))):
            xs += [a + sg * k * math.sqrt(a) for k in GAMMA_SIGMAS for sg in (-1.0, 1.0)]
        if a > 1e8:
            xs += [a + sg * 50.0 * math.sqrt(a) for sg in (-1.0, 1.0)]
            xs += [a * (1.0 + sg * r) for r in GAMMA_WIDE_REL for sg in (-1.0, 1.0)]
        xs += [2.0 ** -126] + ([] if f32 else [2.0 ** -1022])
        for k, x in enumerate(xs):
            x = float(ft(x))
            if x >= tiny and (a, x) not in [p[:2] for p in pts]:
                pts.append((a, x, k < nq))
    out = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    return out + (np.array([p[2] for p in pts]),) if with_quantile_mask else out


def gamma_branch(a, x):
    """Which evaluation csrc/gamma.hip takes at (a, x): 'cornish' (the Cornish-Fisher form: a >= 1e4 within 8
    standard deviations of the mean, and a > 1e8 within a hundredth of the mean), 'series' (x < a + 1) or
    'fraction' (the continued fraction)."""
    a, x = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(x, np.float64))
    d = np.abs(x - a)
    cornish = (a >= 1e4) & ((d <= 8.0 * np.sqrt(a)) | ((a > 1e8) & (d <= 0.01 * a)))
    return np.where(cornish, "cornish", np.where(x < a + 1.0, "series", "fraction"))


def gamma_grad_fixture(f32):
    """(a, x, ref) of the fixture; the stored grid must be the one gamma_grid() makes."""
    z = golden("gamma_grad_edges")
    key = dname(f32)
    return z[key + "/a"], z[key + "/x"], z[key + "/ref"]


def gamma_grad_bound(a, x, ref, f32):
    """The device bound per point: relative, 4 x the host oracle's measured maximum of the point's branch, at
    most 1e-9; float32 adds one rounding of the result.  A result below the dtype's normal range may be flushed."""
    rel = np.array([min(4 * GAMMA_HOST_MAX[b], GAMMA_DEVICE_CAP) for b in gamma_branch(a, x)])
    return (rel + (2.0 ** -23 if f32 else 0.0)) * np.abs(ref) + (F32_TINY if f32 else 2.0 ** -1022)


def gamma_grad_ratios(got, a, x, ref, f32):
    """{branch: largest |got - ref| / bound}."""
    bound = gamma_grad_bound(a, x, ref, f32)
    br = gamma_branch(a, x)
    with np.errstate(all="ignore"):
        ratio = np.where(got == ref, 0.0, np.abs(got - ref) / bound)
    ratio = np.where(np.isfinite(ratio), ratio, INF)
    return {b: float(ratio[br == b].max()) for b in GAMMA_BRANCHES if (br == b).any()}


def gamma_draw_shapes(cus):
    return [(1, 1), (3, 85), (1, adam_grid_stride_n(cus))]


def gamma_draw_alpha(rows, cols, f32):
    """Concentrations in [0.05, 300] (log-uniform) with the points 0.999, 1, 1.001 and 1e4 among them."""
    r = np.random.default_rng(rows * 7919 + cols)
    a = np.exp(r.uniform(math.log(0.05), math.log(300.0), rows * cols))
    a[:: 97] = 1.0
    a[5:: 97] = 0.999
    a[11:: 97] = 1.001
    a[17:: 197] = 1e4
    a = a.reshape(rows, cols)
    return to32(a) if f32 else a


# =======================================================================================================
# full-covariance guide (pa_mvn_tril_sample / _bwd)
# =======================================================================================================
MVN_N = (1, 2, 63, 64, 65, 127, 128, 129, 257)
MVN_P = (1, 2, 4, 5, 8, 9, 12, 13)
MVN_RHO_SPECIALS = (-30.0, 19.999, 20.0, 20.001, 25.0)
MVN_VARIANTS = (None, "ordinary", "underflow", "offset")
LOG_2PI = 1.8378770664093453


def mvn_inputs(n, P, f32, variant=None):
    """(loc [n], rho [n], A [n, n], eps [P, n], d_z [P, n], d_logq [P]) float64 torch tensors, representable in
    the target precision.  rho holds the five values of MVN_RHO_SPECIALS among U(-2, 1.5) (n < 5: as many as
    fit, rotating with P); 'ordinary': none of them; 'underflow': one rho = -200; 'offset': loc = 1e4 and scales
    of about 1e-3."""
    g = torch.Generator().manual_seed(n * 1000 + P)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    loc, A, eps, d_z, d_q = rnd(n), rnd(n, n) * (0.3 / math.sqrt(n)), rnd(P, n), rnd(P, n), rnd(P)
    rho = torch.rand(n, generator=g, dtype=F64) * 3.5 - 2.0
    if variant == "offset":
        loc = loc + 1e4
        rho = math.log(math.expm1(1e-3)) + 0.2 * rnd(n)
    elif variant == "underflow":
        rho[n // 2] = -200.0
    elif variant is None:
        at = [(k * n) // 5 + (n > 5) * 1 for k in range(5)] if n >= 5 else list(range(n))
        for k, i in enumerate(at):
            rho[i] = MVN_RHO_SPECIALS[(k + (P if n < 5 else 0)) % 5]
    elif variant != "ordinary":
        raise ValueError(variant)
    xs = (loc, rho, A, eps, d_z, d_q)
    return tuple(x.float().double() for x in xs) if f32 else xs


def mvn_forward(loc, rho, A, eps, dtype, solve):
    """(z, logq) in ``dtype`` with the graph attached; ``solve``: log q from MultivariateNormal's triangular solve
    (centred, see the docstring), else from eps directly."""
    n = loc.numel()
    S = torch.nn.functional.softplus(rho)
    T = S[:, None] * (A.tril(-1) + torch.eye(n, dtype=dtype))
    u = eps @ T.T
    z = loc + u
    if solve:
        mvn = torch.distributions.MultivariateNormal(torch.zeros(n, dtype=dtype), scale_tril=T, validate_args=False)
        return z, mvn.log_prob(u)
    return z, -0.5 * (eps * eps).sum(-1) - torch.log(S).sum() - 0.5 * n * LOG_2PI


def mvn_reference(inp, dtype, solve, which=(True, True)):
    """(z, logq, d_loc, d_rho, d_A) float64 numpy; ``which`` = (d_z given, d_logq given).  The backward is
    autograd of the direct form of log q whatever ``solve`` says for the forward (see the docstring)."""
    loc, rho, A, eps, d_z, d_q = (x.to(dtype) for x in inp)
    with torch.no_grad():
        z, logq = mvn_forward(loc, rho, A, eps, dtype, solve)
    l, r, a = (x.clone().requires_grad_(True) for x in (loc, rho, A))
    zz, lq = mvn_forward(l, r, a, eps, dtype, False)
    loss = 0.0 * zz.sum()
    if which[0]:
        loss = loss + (zz * d_z).sum()
    if which[1]:
        loss = loss + (lq * d_q).sum()
    loss.backward()
    return tuple(x.detach().double().numpy() for x in (z, logq, l.grad, r.grad, a.grad))


def mvn_magnitudes(inp, z, which=(True, True)):
    """(M_z, M_logq, M_dloc, M_drho, M_dA) float64 numpy; ``z`` = the draw the backward is given."""
    loc, rho, A, eps, d_z, d_q = (x.double() for x in inp)
    n = loc.numel()
    S = torch.nn.functional.softplus(rho)
    L = A.tril(-1).abs()
    Mz = loc.abs() + S * (eps.abs() @ L.T + eps.abs())
    Mq = 0.5 * (eps * eps).sum(-1) + torch.log(S).abs().sum() + 0.5 * n * LOG_2PI
    dz = d_z.abs() if which[0] else torch.zeros_like(d_z)
    dq = d_q.abs() if which[1] else torch.zeros_like(d_q)
    Ml = dz.sum(0)
    sig = torch.where(rho > 20, torch.ones_like(rho), torch.sigmoid(rho))
    Mr = sig * ((dz * (torch.as_tensor(z).abs() + loc.abs())).sum(0) + dq.sum()) / S
    MA = (S[:, None] * (dz.T @ eps.abs())).tril(-1)
    return tuple(x.numpy() for x in (Mz, Mq, Ml, Mr, MA))


@functools.lru_cache(maxsize=None)
def mvn_case(n, P, f32, variant=None, which=(True, True)):
    """dict: inp (float64 tensors), ref / cpu32 = (z, logq, d_loc, d_rho, d_A), M (same order)."""
    inp = mvn_inputs(n, P, f32, variant)
    with np.errstate(all="ignore"):
        ref = mvn_reference(inp, F64, True, which)
        cpu32 = mvn_reference(inp, F32, False, which) if f32 else None
        M = mvn_magnitudes(inp, (cpu32 or ref)[0], which)
    return {"inp": inp, "ref": ref, "cpu32": cpu32, "M": M}


MVN_OUTPUTS = ("z", "logq", "d_loc", "d_rho", "d_A")


def mvn_check(label, got, case, f32, only=None):
    """The rule on the outputs named in ``only`` (default: all five that ``got`` holds, None entries skipped)."""
    c32 = case["cpu32"] or (None,) * 5
    for what, g, r, M, c in zip(MVN_OUTPUTS, got, case["ref"], case["M"], c32):
        if g is not None and (only is None or what in only):
            check(label, what, g, r, M, f32, c)


# =======================================================================================================
# guide_site.hip: exp_site_fwd / _bwd and meanfield_score
# =======================================================================================================
SITE_COLS = (1, 63, 64, 65, 130)
SITE_ROWS = (1, 3, 5)
SITE_LOWER = (0.0, -2.5, 1e6)
SCORE_SHAPES = ((1, 1), (3, 7), (5, 255), (5, 256), (5, 257), (2, 1000), (64, 513))
SCORE_CAP_SHAPE = (64, 65537)        # P * n = 4 194 368, just above the 1024 blocks of 4096 elements
SCORE_COEF = -0.25


def site_loop_rows(cus):
    """A row count above the forward launch's 4 waves x 8 * CUs workgroups: waves loop."""
    return 4 * 8 * cus + 3


def site_inputs(rows, cols, f32):
    """(u [rows, cols], g_value [rows, cols], g_ld [rows]) float64 tensors: u uniform in [-100, 80] with both
    ends present, and, where the case has at least 32 elements, 3 % of them at 89 or 100 (float32 exp
    overflows; under the cap of unscored elements)."""
    g = torch.Generator().manual_seed(rows * 131 + cols)
    n = rows * cols
    u = torch.rand(n, generator=g, dtype=F64) * 180.0 - 100.0
    if n >= 2:
        u[0], u[n - 1] = -100.0, 80.0
    if n >= 32:
        k = max(1, (3 * n) // 100)
        at = torch.randperm(n - 2, generator=g)[:k] + 1
        u[at] = torch.where(torch.arange(k) % 2 == 0, 89.0, 100.0).double()
    gv, gl = torch.randn(n, generator=g, dtype=F64), torch.randn(rows, generator=g, dtype=F64)
    xs = (u.reshape(rows, cols), gv.reshape(rows, cols), gl)
    return tuple(x.float().double() for x in xs) if f32 else xs


def site_forward(u, lower, dtype):
    u = u.to(dtype)
    return lower + torch.exp(u), -u.sum(-1)


def site_backward(value, g_value, g_ld, lower, dtype):
    """d u from the value the backward is GIVEN (as the kernel: value - lower stands for exp(u))."""
    out = torch.zeros_like(value, dtype=dtype)
    if g_value is not None:
        out = out + g_value.to(dtype) * (value.to(dtype) - lower)
    if g_ld is not None:
        out = out - g_ld.to(dtype)[:, None]
    return out


@functools.lru_cache(maxsize=None)
def site_case(rows, cols, lower, f32):
    """dict: u, g_value, g_ld, value_in (what the backward is given: lower + exp(min(u, 80)) in the target
    precision), fwd / fwd32 = (value, ld), M_fwd, and bwd(which) -> (ref, cpu32, M)."""
    u, gv, gl = site_inputs(rows, cols, f32)
    d = dt(f32)
    with np.errstate(all="ignore"):
        fwd = tuple(x.numpy() for x in site_forward(u, lower, F64))
        fwd32 = tuple(x.double().numpy() for x in site_forward(u, lower, F32)) if f32 else None
        value_in = (lower + torch.exp(u.clamp(max=80.0).to(d))).double()
    M_fwd = ((abs(lower) + torch.exp(u)).numpy(), u.abs().sum(-1).numpy())
    return {"u": u, "g_value": gv, "g_ld": gl, "value_in": value_in, "fwd": fwd, "fwd32": fwd32, "M_fwd": M_fwd,
            "lower": lower}


def site_bwd_reference(case, which, f32):
    """(ref64, cpu32 or None, M) of d u with ``which`` = (g_value given, g_ld given)."""
    gv = case["g_value"] if which[0] else None
    gl = case["g_ld"] if which[1] else None
    v, lower = case["value_in"], case["lower"]
    ref = site_backward(v, gv, gl, lower, F64).numpy()
    c32 = site_backward(v, gv, gl, lower, F32).double().numpy() if f32 else None
    M = torch.zeros_like(v)
    if which[0]:
        M = M + gv.abs() * (v.abs() + abs(lower))
    if which[1]:
        M = M + gl.abs()[:, None]
    return ref, c32, M.numpy()


def score_inputs(P, n, f32):
    g = torch.Generator().manual_seed(P * 100003 + n)
    loc = torch.randn(n, generator=g, dtype=F64)
    scale = torch.rand(n, generator=g, dtype=F64) * 1.95 + 0.05
    z = loc + scale * torch.randn(P, n, generator=g, dtype=F64)
    xs = (z, loc, scale)
    return tuple(x.float().double() for x in xs) if f32 else xs


def score_reference(z, loc, scale, coef, dtype):
    z, loc, scale = (x.to(dtype) for x in (z, loc, scale))
    total = torch.distributions.Normal(loc, scale).log_prob(z).sum() * coef
    return total.double().numpy(), (-coef * z.shape[0] / scale).double().numpy()


@functools.lru_cache(maxsize=None)
def score_case(P, n, f32):
    """dict: z, loc, scale, ref / cpu32 = (total, gscale), M = (M_total, M_gscale)."""
    z, loc, scale = score_inputs(P, n, f32)
    ref = score_reference(z, loc, scale, SCORE_COEF, F64)
    cpu32 = score_reference(z, loc, scale, SCORE_COEF, F32) if f32 else None
    e = (z - loc) / scale
    Mt = abs(SCORE_COEF) * float(0.5 * (e * e).sum() + P * scale.log().abs().sum() + P * n * 0.5 * LOG_2PI)
    return {"z": z, "loc": loc, "scale": scale, "ref": ref, "cpu32": cpu32,
            "M": (np.float64(Mt), (abs(SCORE_COEF) * P / scale).numpy())}


def score_check(label, total, gscale, case, f32):
    c32 = case["cpu32"] or (None, None)
    check(label, "total", total, case["ref"][0], case["M"][0], f32, c32[0])
    check(label, "gscale", gscale, case["ref"][1], case["M"][1], f32, c32[1])
