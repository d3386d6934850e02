"""TEST INFRASTRUCTURE -- the fused Gaussian NUTS kernels (pyro_amd/csrc/nuts.hip) tree for tree: the
case tables and the device-independent runners and checks shared by tests/test_nuts_edges_gpu.py (the
HIP kernels) and tests/test_nuts_edges_host.py (the same tables through tests/oracle_backend.py, plus
the conditions the tables have to meet).

Every case is ONE transition of one chain from a fresh state: inputs are drawn in float64 and rounded to
the tensor dtype, the same rounded values go to the kernel and to the oracle, nothing accumulates and
every (chain, t) is an independent case.

float64 cases: oracle/nuts.py with the kernel's keyed Philox draws in float64 arithmetic; the integer
outputs are equal, the floating ones agree to RTOL64.

float32 cases: the same oracle in float64 ARITHMETIC on the float32 DRAWS (the high-precision statement
of the same operation on the same random inputs).  float32 rounding may flip a comparison that sits on
its threshold, so the oracle records how far every decision of a transition was from its threshold
(oracle.nuts.Margins); a case whose margins are all above F32_MARGINS is decidable and has to match in
every integer output and, to F32_TOL, in z / pe / accept_prob; the others are only checked for finite
outputs inside the tree-size limit, and may be at most CAP of the cases of a parametrisation.

F32_DEV is measured, not guessed: the largest |z32 - z64| / (1e-3 + |z64|) between the oracle run in
numpy float32 (potential included) and in float64 over every float32 case of the tables below whose
trees agree (``python -m tests.nuts_edge_cases`` prints it).  The device sums in another order and uses
v_exp_f32 / v_log_f32, hence the factor 4.  The margin is the same tolerance in the units of each margin:
with the one number F32_TOL for every kind, 6.5 % of the cases below are undecidable (a transition of 20
leapfrogs makes some 25 uniform draws, each within 1.7e-3 of its probability once in 300), so the kinds
whose compared quantity is measured in the same two runs use 4 x its own largest deviation (F32_QDEV),
which is smaller: fewer cases are set aside, never more.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import integrator as o_int
from oracle import nuts as o_nuts

SEED = 20240
RTOL64 = 1e-9                 # the project's float64 tolerance for the fused NUTS kernel
F32_DEV = 4.34e-4             # measured: see the module docstring and DESIGN.md "NUTS kernel edge tests"
F32_TOL = 4 * F32_DEV
# Smallest margin a decidable float32 case may have, per kind of decision (oracle.nuts.Margins).  The
# tolerance itself where nothing finer is known; for the kinds below, 4 x the largest deviation of the
# compared quantity itself (the probability cut to [0, 1], the cosine, the sliced energy, delta) between
# the same two oracle runs -- always below F32_TOL, so never more cases are set aside than with the one
# number.  A direction draw is compared with the constant 0.5: no rounding can move it.
F32_QDEV = {"draw": 1.53e-5, "turn": 2.4e-7, "slice": 2.93e-5, "find_step": 1.61e-5}     # measured
F32_MARGINS = {"diverge": F32_TOL, "direction": 0.0}
F32_MARGINS.update({k: min(F32_TOL, 4 * v) for k, v in F32_QDEV.items()})
CAP = 0.02                    # undecidable share allowed per parametrisation
T_TOP = (1 << 43) - 2         # the last transition index the library accepts for a one-transition launch
NUTS_MAX_DEPTH = 10           # nuts_common.h
DPADS = (32, 64, 96, 100, 104, 128)   # nuts_dispatch's ladder of register-kernel instantiations

Row = namedtuple("Row", "D C f32 multinomial depth steps ts chain_offset")
Row.__new__.__defaults__ = ((0,), 0)


def dpad_of(D):
    """The nuts_gaussian_reg_kernel<DPAD> instantiation nuts_dispatch selects for a float32 D."""
    return next(p for p in DPADS if D <= p)


# ---- tables ------------------------------------------------------------------------------------------
# steps = (lo, hi, "lin" | "log"): per-chain step sizes, uniform or log-uniform in [lo, hi]
MODERATE = (0.05, 0.4, "lin")
TINY = (1e-4, 1e-3, "log")            # never turns inside depth <= 10: every chain runs to the limit
MIXED = (1.0, 4.0, "log")             # some chains diverge, some at a later leaf
FIRST_LEAF = (4.0, 300.0, "log")      # every chain diverges at its first leaf
OVERFLOW64 = (1e150, 1e160, "log")    # the energy overflows: NaN -> +inf
OVERFLOW32 = (1e30, 1e38, "log")

D_EDGES_F64 = (1, 2, 63, 64, 65, 127, 128)                  # the 64-lane split and both ends
D_EDGES_F32 = (1, 31, 32, 33, 64, 65, 96, 97, 100, 101, 104, 105, 128)   # both sides of every DPAD step
SAMPLERS = (True, False)              # use_multinomial


def d_edge_rows(D, f32):
    """72 cases per D: both samplers, 12 chains, three transition indices."""
    return [Row(D, 12, f32, mn, 6, MODERATE, (0, 1, 2)) for mn in SAMPLERS]


def c_edge_rows(f32):
    """C = 1, 3, 5: the last workgroup (2 waves in float64, 4 in float32 forced to LDS) has waves with
    chain >= C that leave early.  D = 65 uses both halves of a lane."""
    return [Row(65, C, f32, mn, 5, MODERATE, (0, 1, 2, 3)) for C in (1, 3, 5) for mn in SAMPLERS]


def depth_limit_rows(f32):
    rows = [Row(D, 16, f32, mn, depth, TINY) for depth in (1, 3) for D in (1, 65, 128) for mn in SAMPLERS]
    return rows


DEPTH10_ROWS = [Row(D, 4, False, D == 65, NUTS_MAX_DEPTH, TINY) for D in (65, 128)]   # 1023 leapfrogs each


def divergence_rows(f32):
    over = OVERFLOW32 if f32 else OVERFLOW64
    rows = [Row(D, 16, f32, mn, 6, MIXED, (0, 1)) for D in (1, 2, 65) for mn in SAMPLERS]
    rows += [Row(D, 16, f32, True, 6, FIRST_LEAF) for D in (1, 128)]
    rows += [Row(D, 8, f32, mn, 6, over) for D in (1, 2, 65, 128) for mn in SAMPLERS]
    return rows


def key_rows(f32):
    return [Row(33, 8, f32, mn, 5, MODERATE, (T_TOP,), 1000 + 7 * int(mn)) for mn in SAMPLERS]


def all_rows(f32):
    rows = [r for D in (D_EDGES_F32 if f32 else D_EDGES_F64) for r in d_edge_rows(D, f32)]
    rows += c_edge_rows(f32) + depth_limit_rows(f32) + divergence_rows(f32) + key_rows(f32)
    return rows + ([] if f32 else DEPTH10_ROWS)


# ---- inputs and references -------------------------------------------------------------------------------
def np_dtype(f32):
    return np.float32 if f32 else np.float64


def gauss_lambda(D, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((D, D))
    Lam = np.linalg.inv(A @ A.T / D + 0.1 * np.eye(D))
    return 0.5 * (Lam + Lam.T)


def _steps(rng, spec, C):
    lo, hi, kind = spec
    if kind == "lin":
        return rng.uniform(lo, hi, C)
    return np.exp(rng.uniform(math.log(lo), math.log(hi), C))


@functools.lru_cache(maxsize=None)
def inputs(row):
    """(Lambda, z, pe, grad, inv_mass, step) as numpy arrays of the row's dtype: drawn in float64,
    rounded, pe / grad computed in float64 from the rounded z and Lambda and rounded."""
    dt = np_dtype(row.f32)
    rng = np.random.default_rng([SEED, row.D, row.C, int(row.multinomial), row.depth])
    Lam = gauss_lambda(row.D).astype(dt)
    z = (0.5 * rng.standard_normal((row.C, row.D))).astype(dt)
    im = rng.uniform(0.5, 1.5, (row.C, row.D)).astype(dt)
    with np.errstate(over="ignore"):
        step = _steps(rng, row.steps, row.C).astype(dt)
    assert np.isfinite(step).all()
    g64 = z.astype(np.float64) @ Lam.astype(np.float64)
    pe = (0.5 * (z.astype(np.float64) * g64).sum(1)).astype(dt)
    out = (Lam, z, pe, g64.astype(dt), im, step)
    for a in out:
        a.setflags(write=False)
    return out


def oracle_case(row, c, t, dtype=np.float64, trace=False):
    """One chain of one row through oracle/nuts.py in ``dtype`` arithmetic on the row's draws."""
    Lam, z, pe, g, im, step = inputs(row)
    pg = o_int.gaussian_potential(Lam.astype(dtype))
    mg = o_nuts.Margins(trace)
    with np.errstate(all="ignore"):
        out = o_nuts.nuts_transition(z[c].astype(dtype), float(pe[c]), g[c].astype(dtype), pg,
                                     im[c].astype(dtype), dtype(step[c]),
                                     o_nuts.KeyedDraws(SEED, row.chain_offset + c, t, np_dtype(row.f32)),
                                     row.depth, row.multinomial, dtype=dtype, margins=mg)
    return out, mg


@functools.lru_cache(maxsize=None)
def reference(row):
    """{(t, c): (oracle output, Margins)} -- computed once per row and shared by every test."""
    return {(t, c): oracle_case(row, c, t) for t in row.ts for c in range(row.C)}


def decidable(row, mg):
    return (not row.f32) or all(v > F32_MARGINS[k] for k, v in mg.min.items())


# ---- runners ---------------------------------------------------------------------------------------------
def _t(a, device):
    return torch.as_tensor(np.array(a), device=device).contiguous()


def run_row(k, device, row, through_run=False):
    """The row's transitions through ``k.nuts_gaussian_transition`` (or, with ``through_run``, through
    ``k.nuts_gaussian_run`` with count_accepts and div_flags), every t from the fresh state.
    Returns {t: dict of numpy arrays}."""
    Lam, z, pe, g, im, step = inputs(row)
    got = {}
    for t in row.ts:
        tz, tpe, tg = _t(z, device), _t(pe, device), _t(g, device)
        args = (tz, tpe, tg, _t(Lam, device), _t(im, device), _t(step, device), row.depth,
                row.multinomial, SEED, t)
        if through_run:
            flags = torch.full((1, row.C), -1, dtype=torch.int8, device=device)
            counters = torch.zeros((3, row.C), dtype=torch.int64, device=device)
            out = k.nuts_gaussian_run(*args, 1, chain_offset=row.chain_offset, counters=counters,
                                      count_accepts=True, div_flags=flags)
        else:
            out = k.nuts_gaussian_transition(*args, chain_offset=row.chain_offset)
        res = {n: v.cpu().numpy() for n, v in out.items()}
        res.update(z=tz.cpu().numpy(), pe=tpe.cpu().numpy(), grad=tg.cpu().numpy())
        if through_run:
            res.update(div_flags=flags.cpu().numpy(), counters=counters.cpu().numpy())
        got[t] = res
    return got


def _rel(a, b):
    """|a - b| / (1e-3 + |b|), the normalisation F32_DEV was measured in; 0 where both are the same
    infinity or both NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        return np.where(same, 0.0, np.abs(a - b) / (1e-3 + np.abs(b)))


def check_row(row, got, stats=None):
    """Every (t, chain) of ``got`` against reference(row).  Returns (cases, undecidable)."""
    Lam, z0, pe0, g0, _, _ = inputs(row)
    L64 = Lam.astype(np.float64)
    ref = reference(row)
    tol = F32_TOL if row.f32 else RTOL64
    und = 0
    for t in row.ts:
        r = got[t]
        for c in range(row.C):
            o, mg = ref[(t, c)]
            tag = (row, t, c)
            assert 1 <= r["n_leapfrog"][c] <= (1 << row.depth) - 1, tag
            assert 0 <= r["depth"][c] <= row.depth, tag
            assert r["accepted"][c] in (0, 1) and r["diverging"][c] in (0, 1), tag
            if not r["accepted"][c]:        # state untouched, bit for bit
                assert np.array_equal(r["z"][c], z0[c]) and r["pe"][c] == pe0[c], tag
                assert np.array_equal(r["grad"][c], g0[c]), tag
            else:                           # the gradient of the returned z
                gz = L64 @ r["z"][c].astype(np.float64)
                bound = tol * (1e-3 + np.abs(L64) @ np.abs(r["z"][c].astype(np.float64)))
                assert (np.abs(r["grad"][c] - gz) <= bound).all(), tag
            if "div_flags" in r:
                assert r["div_flags"][0, c] == r["diverging"][c], tag
                assert tuple(r["counters"][:, c]) == (r["n_leapfrog"][c], r["depth"][c], r["accepted"][c]), tag
            if not decidable(row, mg):
                und += 1
                assert np.isfinite(r["z"][c]).all() and np.isfinite(r["grad"][c]).all(), tag
                assert np.isfinite(r["pe"][c]) and np.isfinite(r["accept_prob"][c]), tag
                continue
            assert r["n_leapfrog"][c] == o["n_leapfrog"] and r["depth"][c] == o["depth"], \
                (tag, r["n_leapfrog"][c], o["n_leapfrog"], r["depth"][c], o["depth"])
            assert bool(r["accepted"][c]) == o["accepted"], tag
            assert bool(r["diverging"][c]) == o["diverging"], tag
            if o["diverging"] and not o["accepted"]:
                assert np.array_equal(r["z"][c], z0[c]) and r["pe"][c] == pe0[c], tag
            errs = {"z": _rel(r["z"][c], o["z"]).max(), "pe": float(_rel(r["pe"][c], o["pe"])),
                    "accept_prob": float(_rel(r["accept_prob"][c], o["accept_prob"]))}
            if not row.f32:
                errs["grad"] = _rel(r["grad"][c], o["grad"]).max()
            for n, e in errs.items():
                if stats is not None:
                    stats[n] = max(stats.get(n, 0.0), float(e))
                assert e <= tol, (tag, n, e)
    return len(row.ts) * row.C, und


def check_rows(k, device, rows, through_run=False, stats=None):
    """Runs and checks the rows of one parametrisation and holds the undecidable share to CAP."""
    n = und = 0
    for row in rows:
        a, b = check_row(row, run_row(k, device, row, through_run), stats)
        n, und = n + a, und + b
    assert und <= CAP * n, "undecidable share %d / %d above %g" % (und, n, CAP)
    return n, und


# ---- find_step ---------------------------------------------------------------------------------------------
FS_SEED, FS_KEY, FS_OFFSET = 77, (1 << 42) + 256, 3
FS_THRESHOLD = math.log(0.8)
FS_D = (1, 64, 65, 128)
FS_C = 8
# name: (start, min_step, max_step, one NaN in z, inv_mass per row).  The bounds are powers of two, so
# float32 and float64 hold the same numbers.
FS_CASES = {
    "up": (1e-3, 2.0 ** -30, 2.0 ** 30, False, True),
    "near": (1.0, 2.0 ** -30, 2.0 ** 30, False, True),
    "down": (50.0, 2.0 ** -30, 2.0 ** 30, False, True),
    "clamp_hi": (1e-3, 2.0 ** -30, 2.0 ** -7, False, True),      # doubles past max_step: clamped
    "clamp_lo": (50.0, 8.0, 2.0 ** 30, False, True),             # halves past min_step: clamped
    "outside_lo": (1e-3, 2.0 ** -4, 2.0 ** 4, False, True),      # no trial after the first
    "outside_hi": (50.0, 2.0 ** -4, 2.0 ** 4, False, True),
    "nan": (1.0, 2.0 ** -12, 2.0 ** 30, True, True),             # direction -1 down to min_step
    "broadcast": (1.0, 2.0 ** -30, 2.0 ** 30, False, False),     # inv_mass [D] for every chain
}


@functools.lru_cache(maxsize=None)
def fs_inputs(name, D, f32):
    start, lo, hi, nan, per_row = FS_CASES[name]
    dt = np_dtype(f32)
    rng = np.random.default_rng([SEED, 9, D, sorted(FS_CASES).index(name)])
    Lam = gauss_lambda(D).astype(dt)
    z = (0.5 * rng.standard_normal((FS_C, D))).astype(dt)
    im = rng.uniform(0.5, 1.5, (FS_C, D) if per_row else (D,)).astype(dt)
    step = (start * np.exp(rng.uniform(-0.3, 0.3, FS_C))).astype(dt)
    if nan:
        z[np.arange(FS_C), np.arange(FS_C) % D] = np.nan
    with np.errstate(all="ignore"):
        g64 = z.astype(np.float64) @ Lam.astype(np.float64)
        pe = (0.5 * (z.astype(np.float64) * g64).sum(1)).astype(dt)
    return Lam, z, pe, g64.astype(dt), im, step, lo, hi


@functools.lru_cache(maxsize=None)
def fs_reference(name, D, f32):
    """[(step, trials, smallest |threshold + delta|)] per chain: float64 arithmetic, the dtype's draws."""
    Lam, z, pe, g, im, step, lo, hi = fs_inputs(name, D, f32)
    out = []
    for c in range(FS_C):
        mg = o_nuts.Margins()
        s, n = o_nuts.find_step_gaussian(z[c], pe[c], g[c], Lam, im[c] if im.ndim == 2 else im, step[c],
                                         FS_SEED, FS_KEY, FS_OFFSET + c, lo, hi, FS_THRESHOLD,
                                         np.float64, draw_dtype=np_dtype(f32), margins=mg)
        out.append((float(s), n, mg.smallest()))
    return out


def fs_run(k, device, name, D, f32):
    Lam, z, pe, g, im, step, lo, hi = fs_inputs(name, D, f32)
    out = k.nuts_gaussian_find_step(_t(z, device), _t(pe, device), _t(g, device), _t(Lam, device),
                                    _t(im, device), _t(step, device), FS_SEED, FS_KEY, FS_OFFSET, lo, hi,
                                    FS_THRESHOLD)
    return out.cpu().numpy()


def fs_check(name, D, f32, got):
    """Exact: the result is the start times a power of two (or a bound).  Returns (cases, undecidable)."""
    step, lo, hi = fs_inputs(name, D, f32)[5:]
    und = 0
    for c, (s, n, margin) in enumerate(fs_reference(name, D, f32)):
        tag = (name, D, f32, c, float(got[c]), s, n)
        assert got.dtype == step.dtype and math.isfinite(got[c]) and lo <= got[c] <= hi, tag
        if f32 and margin <= F32_MARGINS["find_step"]:
            und += 1
            if lo < got[c] < hi:            # still the start times a power of two
                assert math.frexp(float(got[c]) / float(step[c]))[0] == 0.5, tag
            continue
        assert float(got[c]) == s, tag
    return FS_C, und


# ---- in-kernel adaptation -----------------------------------------------------------------------------------
ADAPT_C, ADAPT_K, ADAPT_DEPTH, ADAPT_T0 = 5, 6, 5, 40
ADAPT_TARGET = 0.8
ADAPT_WF_N0, ADAPT_MEAN_N0 = 11, 4
ADAPT_ROWS = {3: (0.1, 0.3), 65: (0.1, 0.3), 128: (1.0, 4.0)}     # D: step range (128: divergences)


def dual_averaging_step(da, g, t0=10.0, kappa=0.75, gamma=0.05):
    """DualAveraging.step (pyro/ops/dual_averaging.py:55-78) on one row [x_avg, g_avg, t, prox, x_t]."""
    x_avg, g_avg, t, prox, _ = da
    t = t + 1
    g_avg = (1 - 1 / (t + t0)) * g_avg + g / (t + t0)
    x_t = prox - math.sqrt(t) / gamma * g_avg
    w = t ** (-kappa)
    return np.array([(1 - w) * x_avg + w * x_t, g_avg, t, prox, x_t])


def welford_update(mean, m2, n, z):
    """WelfordCovariance.update, diagonal (pyro/ops/welford.py:27-38); ``n`` counts this sample."""
    pre = z - mean
    mean = mean + pre / n
    return mean, m2 + pre * (z - mean)


@functools.lru_cache(maxsize=None)
def adapt_inputs(D):
    rng = np.random.default_rng([SEED, 11, D])
    C = ADAPT_C
    Lam = gauss_lambda(D)
    z = 0.5 * rng.standard_normal((C, D))
    im = rng.uniform(0.5, 1.5, (C, D))
    step = rng.uniform(*ADAPT_ROWS[D], C)
    step[0] = 1e12                                  # diverges at the first leaf of every transition
    da = np.stack([rng.normal(-1.5, 0.2, C), rng.normal(0.0, 0.05, C), np.full(C, 7.0),
                   np.log(10 * step), np.log(step)], axis=1)
    wf = np.stack([0.3 * rng.standard_normal((C, D)), rng.uniform(0.5, 5.0, (C, D))], axis=1)
    mean_ap = rng.uniform(0.3, 0.9, C)
    g = z @ Lam
    return Lam, z, 0.5 * (z * g).sum(1), g, im, step, da, wf, mean_ap


@functools.lru_cache(maxsize=None)
def adapt_reference(D):
    """The oracle stepped K transitions per chain, each continuing from the last, the step re-derived by
    the dual averaging restated above from the oracle's own accept_prob."""
    Lam, z, pe, g, im, step, da, wf, mean_ap = adapt_inputs(D)
    C, K = ADAPT_C, ADAPT_K
    pg = o_int.gaussian_potential(Lam)
    ref = dict(z=z.copy(), pe=pe.copy(), grad=g.copy(), step=step.copy(), da=da.copy(), wf=wf.copy(),
               mean_ap=mean_ap.copy(), samples=np.zeros((K, C, D)), counters=np.zeros((3, C), np.int64),
               div=np.zeros((K, C), np.int8), last=[None] * C)
    for c in range(C):
        for kk in range(K):
            with np.errstate(all="ignore"):
                o = o_nuts.nuts_transition(ref["z"][c], float(ref["pe"][c]), ref["grad"][c], pg, im[c],
                                           ref["step"][c],
                                           o_nuts.KeyedDraws(SEED, c, ADAPT_T0 + kk, np.float64),
                                           ADAPT_DEPTH, True)
            ref["z"][c], ref["pe"][c], ref["grad"][c] = o["z"], o["pe"], o["grad"]
            ap = 0.0 if o["accept_prob"] != o["accept_prob"] else o["accept_prob"]
            ref["mean_ap"][c] += (ap - ref["mean_ap"][c]) / (ADAPT_MEAN_N0 + kk + 1)
            ref["da"][c] = dual_averaging_step(ref["da"][c], ADAPT_TARGET - ap)
            ref["step"][c] = math.exp(ref["da"][c][4])
            ref["wf"][c] = welford_update(ref["wf"][c, 0], ref["wf"][c, 1], ADAPT_WF_N0 + kk + 1, o["z"])
            ref["samples"][kk, c] = o["z"]
            ref["counters"][:, c] += (o["n_leapfrog"], o["depth"], int(o["accepted"]))
            ref["div"][kk, c] = int(o["diverging"])
            ref["last"][c] = o
    return ref


def adapt_run(k, device, D, count_accepts):
    Lam, z, pe, g, im, step, da, wf, mean_ap = adapt_inputs(D)
    C, K = ADAPT_C, ADAPT_K
    t = {n: _t(v, device) for n, v in dict(z=z, pe=pe, grad=g, step=step, da=da, wf=wf,
                                           mean_ap=mean_ap).items()}
    t["samples"] = torch.zeros((K, C, D), dtype=torch.float64, device=device)
    t["counters"] = _t(np.arange(3 * C, dtype=np.int64).reshape(3, C) + 100, device)   # += : not zero
    t["div"] = torch.full((K, C), -1, dtype=torch.int8, device=device)
    out = k.nuts_gaussian_run(t["z"], t["pe"], t["grad"], _t(Lam, device), _t(im, device), t["step"],
                              ADAPT_DEPTH, True, SEED, ADAPT_T0, K, da_state=t["da"],
                              target_accept=ADAPT_TARGET, welford=t["wf"], welford_n0=ADAPT_WF_N0,
                              samples=t["samples"], mean_accept=t["mean_ap"], mean_n0=ADAPT_MEAN_N0,
                              counters=t["counters"], count_accepts=count_accepts, div_flags=t["div"])
    got = {n: v.cpu().numpy() for n, v in t.items()}
    got["out"] = {n: v.cpu().numpy() for n, v in out.items()}
    return got


def adapt_check(D, got, count_accepts):
    ref = adapt_reference(D)
    da0 = adapt_inputs(D)[6]
    C = ADAPT_C
    close = functools.partial(np.testing.assert_allclose, rtol=RTOL64, atol=RTOL64)
    assert ref["div"][:, 0].all() and (ref["samples"][:, 0] == adapt_inputs(D)[1][0]).all()
    close(got["step"], ref["step"])
    close(got["da"], ref["da"])
    assert np.array_equal(got["da"][:, 3], da0[:, 3])            # prox_center: untouched bit for bit
    assert np.array_equal(got["da"][:, 2], da0[:, 2] + ADAPT_K)
    close(got["wf"], ref["wf"])
    close(got["mean_ap"], ref["mean_ap"])
    close(got["samples"], ref["samples"])
    close(got["z"], ref["z"])
    close(got["pe"], ref["pe"])
    close(got["grad"], ref["grad"])
    base = np.arange(3 * C, dtype=np.int64).reshape(3, C) + 100
    assert np.array_equal(got["counters"][:2], base[:2] + ref["counters"][:2])
    if count_accepts:
        assert np.array_equal(got["counters"][2], base[2] + ref["counters"][2])
        assert np.array_equal(got["div"], ref["div"])                 # [K, C]
    else:
        assert np.array_equal(got["counters"][2], base[2])            # untouched
        assert (got["div"] == -1).all()
    for c in range(C):                                               # the last transition's statistics
        o = ref["last"][c]
        assert got["out"]["n_leapfrog"][c] == o["n_leapfrog"] and got["out"]["depth"][c] == o["depth"]
        assert bool(got["out"]["diverging"][c]) == o["diverging"]
        assert bool(got["out"]["accepted"][c]) == o["accepted"]
        close(got["out"]["accept_prob"][c], o["accept_prob"])


# ---- the float32 measurement -----------------------------------------------------------------------------
def _qdev(kind, a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        return 0.0
    if kind == "draw":                       # u < 1: a probability above 1 decides like 1
        a, b = min(a, 1.0), min(b, 1.0)
    if kind in ("find_step", "diverge") and abs(b) > 10.0:
        return 0.0        # delta far from log(0.8); sliced far from 0 (the "slice" test of the slice sampler)
    return abs(a - b)


def measure_f32_oracle(rows=None):
    """The oracle in numpy float32 (potential included) against the float64 oracle on the float32 rows:
    the largest normalised deviation of z / pe / accept_prob and the largest deviation of every compared
    quantity over the cases whose trees agree, the number of cases whose integer outputs differ and how
    many of those the margins call decidable, and the undecidable share."""
    res = dict(cases=0, undecidable=0, differ=0, differ_decidable=0, z=0.0, pe=0.0, accept_prob=0.0,
               quantities={})
    for row in rows if rows is not None else all_rows(True):
        for t in row.ts:
            for c in range(row.C):
                o, mg = oracle_case(row, c, t, np.float64, trace=True)
                o32, mg32 = oracle_case(row, c, t, np.float32, trace=True)
                res["cases"] += 1
                dec = decidable(row, mg)
                res["undecidable"] += not dec
                ints = ("n_leapfrog", "depth", "accepted", "diverging")
                if any(o32[n] != o[n] for n in ints):
                    res["differ"] += 1
                    res["differ_decidable"] += dec
                    continue
                res["z"] = max(res["z"], float(_rel(o32["z"], o["z"]).max()))
                res["pe"] = max(res["pe"], float(_rel(o32["pe"], o["pe"])))
                res["accept_prob"] = max(res["accept_prob"],
                                         float(_rel(o32["accept_prob"], o["accept_prob"])))
                assert [k for k, _ in mg.trace] == [k for k, _ in mg32.trace]
                for (kind, a), (_, b) in zip(mg32.trace, mg.trace):
                    res["quantities"][kind] = max(res["quantities"].get(kind, 0.0), _qdev(kind, a, b))
    return res


def measure_f32_find_step():
    """The same for the step-size search: the largest deviation of delta near its threshold, the chains
    whose float32 search ends elsewhere, and the undecidable share."""
    res = dict(cases=0, undecidable=0, differ=0, differ_decidable=0, delta=0.0)
    for name in sorted(FS_CASES):
        for D in FS_D:
            Lam, z, pe, g, im, step, lo, hi = fs_inputs(name, D, True)
            for c, (s, n, margin) in enumerate(fs_reference(name, D, True)):
                tr = []
                for dt in (np.float32, np.float64):
                    mg = o_nuts.Margins(trace=True)
                    out = o_nuts.find_step_gaussian(z[c], pe[c], g[c], Lam, im[c] if im.ndim == 2 else im,
                                                    step[c], FS_SEED, FS_KEY, FS_OFFSET + c, lo, hi,
                                                    FS_THRESHOLD, dt, draw_dtype=np.float32, margins=mg)
                    tr.append((float(out[0]), mg.trace))
                res["cases"] += 1
                dec = margin > F32_MARGINS["find_step"]
                res["undecidable"] += not dec
                if tr[0][0] != tr[1][0]:
                    res["differ"] += 1
                    res["differ_decidable"] += dec
                    continue
                for (_, a), (_, b) in zip(*[x[1] for x in tr]):
                    res["delta"] = max(res["delta"], _qdev("find_step", a, b))
    return res


if __name__ == "__main__":
    print(measure_f32_oracle())
    print(measure_f32_find_step())
