"""Launch-path and edge grids of the three enumeration kernels (csrc/logchain.hip, csrc/logsumexp.hip,
csrc/lda.hip), their float64 references and the one tolerance rule that test_enum_edges_host.py (the
numpy oracles) and test_enum_edges_gpu.py (the HIP kernels) share.

References (float64 torch on the CPU, independent of the kernels and of oracle/):
  chain      K**T <= 4096: every path enumerated; logZ = torch.logsumexp of the path scores, gamma and
             xi = ratios of path sums (0 where logZ = -inf: an impossible chain has no posterior, the
             sum-product convention of test_logsumexp_terms_nan_and_inf_follow_torch).  Larger shapes:
             tests/oracle_backend.logchain_fwd_bwd, which the host test pins to the enumeration on
             every small case of the grid.
  lse        torch.logsumexp(sum of the broadcast terms, rdim) and its autograd; G = 0 on an all -inf
             column (same convention).
  lda        out[b] = sum_w logsumexp_t(lt[b, t] + lp[t, words[w, b]]); responsibilities = softmax over
             t per (word, document) pair, 0 for a pair whose logsumexp is -inf, scattered into g_theta
             and g_phi.

Tolerance (one rule, every path; the "f32 class" rule of tests/dist_edge_cases.py):
  float64  the non-finite pattern (NaN, +inf, -inf) equals the reference's exactly; elsewhere
           |got - ref64| <= 64 eps64 M.
  float32  |got - ref64| <= 4 |cpu32 - ref64| + 8 eps32 M, cpu32 = the same plain torch formula
           evaluated in float32 on the CPU (the reference's own f32 error, never the kernel's).  Where
           ref64 is not finite and cpu32 agrees with it, the kernel must give that value exactly.
           Elements where cpu32 is non-finite while ref64 is finite are not scored: at most 5 % of a
           case (UNSCORED_CAP, asserted).  A result below the f32 normal range (2^-126) may be flushed
           to zero.
  M        the magnitude of what was summed:
           - a log-sum-exp output: the float64 sum of |term_k| at the maximising assignment, plus ln of
             the number of reduced entries;
           - logZ of a chain: the sum of those over t, i.e. sum_t |u_t| + sum_t |P_t| along the best
             (Viterbi) path plus T ln K;
           - a document's out: the sum of those over its words (a pair's M = |lt| + |lp| at its best
             topic plus ln T);
           - posteriors and responsibilities (in [0, 1]): an absolute bound with the M of the
             log-normaliser they were divided by; an lse gradient that M times |g_out|;
           - g_theta / g_phi entries (sums of responsibilities): the sum of the pairs' M over the pairs
             summed into the entry.

Largest error / bound per kernel, path and dtype, measured on the MI355X by test_enum_edges_gpu.py
(every case of the module; 1.0 would be the bound):
  chain/generic/f32            0.052
  chain/generic/f64            0.011
  chain/lanes16_D8/f32         0.168
  chain/lanes16_D8/f64         0.022
  chain/lanes32_D2/f64         0.011
  chain/lanes32_D4/f32         0.106
  lda/atomic/TMAX16/f32        0.080
  lda/atomic/TMAX16/f64        0.016
  lda/atomic/TMAX32/f32        0.080
  lda/atomic/TMAX32/f64        0.015
  lda/atomic/TMAX64/f32        0.085
  lda/atomic/TMAX64/f64        0.011
  lda/atomic/TMAX8/f32         0.082
  lda/atomic/TMAX8/f64         0.018
  lda/indexed/TMAX16/f32       0.099
  lda/indexed/TMAX16/f64       0.018
  lda/indexed/TMAX32/f32       0.080
  lda/indexed/TMAX32/f64       0.010
  lda/indexed/TMAX64/f32       0.074
  lda/indexed/TMAX64/f64       0.011
  lda/indexed/TMAX8/f32        0.085
  lda/indexed/TMAX8/f64        0.019
  lse/f32                      0.179
  lse/f64                      0.018
"""
import functools
import math

import numpy as np
import torch

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
F32_TINY = float(np.finfo(np.float32).tiny)
UNSCORED_CAP = 0.05
INF, NAN = math.inf, math.nan
F32, F64 = torch.float32, torch.float64

RATIOS = {}          # label -> largest error / bound seen by check() in this process


# ---- the rule ----------------------------------------------------------------------------------------

def unscored_fraction(ref64, cpu32):
    ref64, cpu32 = np.asarray(ref64, np.float64), np.asarray(cpu32, np.float64)
    if ref64.size == 0:
        return 0.0
    return float((np.isfinite(ref64) & ~np.isfinite(cpu32)).sum()) / ref64.size


def check(label, what, got, ref64, M, f32, cpu32=None, skip=None):
    """Assert the module's rule on one output; ``skip`` masks elements the case does not score (the
    gradients of a +inf / NaN chain).  Records error / bound under ``label``; returns the bound per
    element (inf where the element is not scored)."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, "%s: shape %s, reference %s" % (what, got.shape, ref64.shape)
    M = np.broadcast_to(np.asarray(M, np.float64), got.shape)
    keep = np.ones(got.shape, bool) if skip is None else ~np.broadcast_to(skip, got.shape)
    def kind(x):
        return np.isnan(x) * 1 + (x == INF) * 2 + (x == -INF) * 3

    with np.errstate(all="ignore"):
        fin = np.isfinite(ref64)
        err = np.where(got == ref64, 0.0, np.abs(got - ref64))
        if not f32:
            bound = 64 * EPS64 * M
            scored = keep
        else:
            cpu32 = np.asarray(cpu32, np.float64)
            frac = unscored_fraction(ref64[keep], cpu32[keep])
            assert frac <= UNSCORED_CAP, "%s: %.1f %% of the elements unscored" % (what, 100 * frac)
            bound = 4 * np.abs(cpu32 - ref64) + 8 * EPS32 * M + F32_TINY
            scored = keep & (kind(cpu32) == kind(ref64))
        bad = scored & np.where(fin, ~(np.isfinite(got) & (err <= bound)), kind(got) != kind(ref64))
        ratio = np.where(scored & fin & np.isfinite(got), err / np.where(bound > 0, bound, 1.0), 0.0)
    if ratio.size:
        RATIOS[label] = max(RATIOS.get(label, 0.0), float(ratio.max()))
    idx = np.flatnonzero(bad.ravel())
    lines = ["  [%d] got %.17g ref %.17g bound %.3g" % (i, got.ravel()[i], ref64.ravel()[i],
                                                        np.broadcast_to(bound, got.shape).ravel()[i])
             for i in idx[:8]]
    assert idx.size == 0, "%s %s: %d of %d elements out of tolerance\n%s" % (label, what, idx.size, got.size,
                                                                             "\n".join(lines))
    return np.where(scored & fin, np.broadcast_to(bound, got.shape), INF)


def ratio_table():
    return "\n".join("  %-28s %.3f" % (k, v) for k, v in sorted(RATIOS.items()))


# =======================================================================================================
# chain (pa_logchain_fwd_bwd)
# =======================================================================================================
LC_MAXK = 64
BRUTE_PATHS = 4096
CHAIN_K = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)
CHAIN_LAYOUTS = ("BTKK", "TKK", "KK")
CHAIN_B = (1, 3)


def chain_body(K, T, f32):
    """(body, prefetch depth) the launcher of csrc/logchain.hip picks."""
    if T == 1 or K > 32:
        return "generic", 0
    if K <= 16:
        return "lanes16", 8
    return ("lanes32", 4) if f32 else ("lanes32", 2)


def chain_T(K, f32):
    """The step counts that straddle the prefetch depth of the body K lands on."""
    if K <= 16:
        return (2, 8, 9, 10, 17)
    if K <= 32:
        return (2, 4, 5, 6, 9) if f32 else (2, 3, 4, 5)
    return (2, 3)


def chain_grid(f32):
    """[(K, T)] of the plain grid; every entry runs at every B of CHAIN_B and layout of CHAIN_LAYOUTS."""
    g = [(K, T) for K in CHAIN_K for T in chain_T(K, f32)]
    return g + [(K, 1) for K in (1, 5, 40)]


def chain_pattern_shapes(f32):
    """One small (enumerable) and one prefetch-boundary shape per body."""
    return [(3, 4), (16, 9), (17, 2), (32, 5) if f32 else (32, 3), (33, 2), (64, 3)]


CHAIN_PATTERNS = ("neg_unary", "dead_end", "dead_batch", "scale1e4", "shift3e4", "nan", "pinf1", "pinf2")


def _round_to(x, f32):
    return x.float().double() if f32 else x


def chain_inputs(K, T, B, layout, f32, pattern=None):
    """(U [B,T,K], P in ``layout``) float64, representable in the target precision.  P is never
    symmetric (a transposed xi must not hide)."""
    g = torch.Generator().manual_seed(K * 1000 + T * 10 + B + 7 * CHAIN_LAYOUTS.index(layout))
    U = torch.randn(B, T, K, generator=g, dtype=F64)
    shape = {"BTKK": (B, max(T - 1, 0), K, K), "TKK": (max(T - 1, 0), K, K), "KK": (K, K)}[layout]
    P = torch.randn(shape, generator=g, dtype=F64)
    if K > 1:
        P = P + 0.5 * torch.triu(torch.ones(K, K, dtype=F64), 1)       # upper half shifted: P != P^T
    tm, b1 = T // 2, min(1, B - 1)
    if pattern == "neg_unary":
        U[:, tm, K // 2] = -INF
    elif pattern == "dead_end":                      # a dead-end row and an unreachable column
        P[..., 0, 0, :] = -INF
        P[..., -1, :, 1] = -INF
    elif pattern == "dead_batch":
        U[b1, tm, :] = -INF
    elif pattern == "scale1e4":
        U, P = U * 1e4, P * 1e4
    elif pattern == "shift3e4":
        U = U + 3e4
    elif pattern == "nan":
        U[b1, tm, K // 2] = NAN
    elif pattern == "pinf1":
        U[b1, tm, K // 2] = INF
    elif pattern == "pinf2":
        U[b1, tm, K // 2] = INF
        U[b1, tm, 0] = INF
    elif pattern is not None:
        raise ValueError(pattern)
    return _round_to(U, f32), _round_to(P, f32)


def chain_clean_of(pattern):
    """True where the pattern poisons batch element min(1, B-1) only and the others must be
    bit-identical to the run without it."""
    return pattern in ("dead_batch", "nan", "pinf1", "pinf2")


def chain_expand(P, B, T, K):
    return P.expand(B, max(T - 1, 0), K, K)


def chain_brute(U, P, dtype=F64):
    """Every path enumerated in ``dtype``: (logZ [B], gamma [B,T,K], xi [B,T-1,K,K])."""
    U = U.to(dtype)
    B, T, K = U.shape
    P = chain_expand(P.to(dtype), B, T, K)
    paths = torch.cartesian_prod(*[torch.arange(K)] * T).reshape(-1, T)           # [N, T]
    N = paths.shape[0]
    score = torch.zeros(B, N, dtype=dtype)
    for t in range(T):
        score = score + U[:, t, paths[:, t]]
    for t in range(T - 1):
        score = score + P[:, t, paths[:, t], paths[:, t + 1]]
    lz = torch.logsumexp(score, 1)
    w = torch.exp(score - lz[:, None])
    w = torch.where((lz == -INF)[:, None], torch.zeros_like(w), w)
    gamma = torch.zeros(B, T, K, dtype=dtype)
    xi = torch.zeros(B, max(T - 1, 0), K * K, dtype=dtype)
    for t in range(T):
        gamma[:, t].index_add_(1, paths[:, t], w)
    for t in range(T - 1):
        xi[:, t].index_add_(1, paths[:, t] * K + paths[:, t + 1], w)
    return lz, gamma, xi.reshape(B, max(T - 1, 0), K, K)


def chain_recursion(U, P, dtype):
    """The forward-backward recursion in plain torch in ``dtype`` (the f32 comparison of the shapes
    too large to enumerate): same formula as tests/oracle_backend.logchain_fwd_bwd."""
    U = U.to(dtype)
    B, T, K = U.shape
    P = chain_expand(P.to(dtype), B, T, K)
    alpha = [U[:, 0]]
    for t in range(1, T):
        alpha.append(U[:, t] + torch.logsumexp(alpha[-1][:, :, None] + P[:, t - 1], 1))
    lz = torch.logsumexp(alpha[-1], 1)
    beta = [torch.zeros(B, K, dtype=dtype)]
    xi = []
    for t in range(T - 2, -1, -1):
        w = U[:, t + 1] + beta[0]
        xi.insert(0, torch.exp(alpha[t][:, :, None] + P[:, t] + w[:, None, :] - lz[:, None, None]))
        beta.insert(0, torch.logsumexp(P[:, t] + w[:, None, :], 2))
    gamma = torch.exp(torch.stack(alpha, 1) + torch.stack(beta, 1) - lz[:, None, None])
    xi = torch.stack(xi, 1) if xi else torch.zeros(B, 0, K, K, dtype=dtype)
    dead = lz == -INF
    gamma = torch.where(dead[:, None, None], torch.zeros_like(gamma), gamma)
    xi = torch.where(dead[:, None, None, None], torch.zeros_like(xi), xi)
    return lz, gamma, xi


def chain_magnitude(U, P):
    """M of logZ per batch element [B]: |u| and |P| summed along the best path, plus T ln K."""
    B, T, K = U.shape
    P = chain_expand(P, B, T, K)
    fin = lambda x: torch.nan_to_num(x, nan=-INF, posinf=-INF)      # noqa: E731   (a path that exists)
    Uf, Pf = fin(U), fin(P)
    best, mag = Uf[:, 0], torch.nan_to_num(Uf[:, 0].abs(), posinf=0.0)
    for t in range(1, T):
        cand = best[:, :, None] + Pf[:, t - 1]                                    # [B, i, j]
        top, arg = cand.max(1)
        pm = torch.nan_to_num(Pf[:, t - 1].abs(), posinf=0.0)
        mag = torch.gather(mag[:, :, None] + pm, 1, arg[:, None, :])[:, 0]
        best = top + Uf[:, t]
        mag = mag + torch.nan_to_num(Uf[:, t].abs(), posinf=0.0)
    j = best.argmax(1)
    return torch.gather(mag, 1, j[:, None])[:, 0] + T * math.log(K)


@functools.lru_cache(maxsize=None)
def chain_case(K, T, B, layout, f32, pattern=None):
    """dict of the case: inputs U, P (float64), ref = (logZ, gamma, xi) float64, cpu32 (f32 cases),
    M [B], brute (bool)."""
    from tests import oracle_backend as ob
    U, P = chain_inputs(K, T, B, layout, f32, pattern)
    brute = K ** T <= BRUTE_PATHS
    with np.errstate(all="ignore"):
        ref = chain_brute(U, P) if brute else ob.logchain_fwd_bwd(U, P)
        cpu32 = None
        if f32:
            cpu32 = chain_brute(U, P, F32) if brute else chain_recursion(U, P, F32)
            cpu32 = tuple(x.double().numpy() for x in cpu32)
    return {"U": U, "P": P, "ref": tuple(x.double().numpy() for x in ref), "cpu32": cpu32,
            "M": chain_magnitude(U, P).numpy(), "brute": brute}


def chain_check(label, got, case, f32, pattern=None):
    """The rule on (logZ, gamma, xi) and, on finite chains, the two marginal properties."""
    lz, gamma, xi = (np.asarray(x, np.float64) for x in got)
    rlz, rg, rx = case["ref"]
    c32 = case["cpu32"] or (None, None, None)
    M = case["M"]
    # the gradients of a chain whose logZ is +inf or NaN are not scored
    skipb = ~np.isfinite(rlz) & ~(rlz == -INF)
    check(label, "logZ", lz, rlz, M, f32, c32[0])
    bg = check(label, "gamma", gamma, rg, M[:, None, None], f32, c32[1], skip=skipb[:, None, None])
    bx = check(label, "xi", xi, rx, M[:, None, None, None], f32, c32[2], skip=skipb[:, None, None, None])
    # gamma sums to 1, xi's marginals are gamma_t and gamma_{t+1}: within the summed element bounds
    ok = np.isfinite(rlz)
    rnd = gamma.shape[-1] * EPS64
    assert (np.abs(gamma[ok].sum(-1) - 1) <= bg[ok].sum(-1) + rnd).all(), "%s: gamma does not sum to 1" % label
    if xi.shape[1]:
        assert (np.abs(xi[ok].sum(-1) - gamma[ok][:, :-1]) <= bx[ok].sum(-1) + bg[ok][:, :-1] + rnd).all(), \
            "%s: xi summed over the next state is not gamma_t" % label
        assert (np.abs(xi[ok].sum(-2) - gamma[ok][:, 1:]) <= bx[ok].sum(-2) + bg[ok][:, 1:] + rnd).all(), \
            "%s: xi summed over the current state is not gamma_{t+1}" % label


# =======================================================================================================
# logsumexp_terms / _grad
# =======================================================================================================

def _lse_frames():
    out = []
    for kept in (255, 256, 257):
        a, b = {255: (15, 17), 256: (16, 16), 257: (257, 1)}[kept]
        for R in (1, 2, 1000):
            out.append(("k%d_r%d_first" % (kept, R), (R, kept), 0, [(R, kept), (R, 1)]))
            out.append(("k%d_r%d_mid" % (kept, R), (a, R, b), 1, [(a, R, b), (1, R, b), (a, 1, 1)]))
            out.append(("k%d_r%d_last" % (kept, R), (kept, R), 1, [(kept, R), (1, R)]))
    return out


def lse_names():
    return [c[0] for c in _lse_frames()] + ["max_terms_dims", "strided", "cancel"]


def lse_inputs(name, f32):
    """(terms, frame, rdim): a term is a float64 tensor or (base tensor, view recipe) -- see lse_view;
    the kernels read the view's own strides."""
    from pyro_amd import _lib
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *sh: _round_to(3 * torch.randn(*sh, generator=g, dtype=F64), f32)   # noqa: E731
    if name == "max_terms_dims":
        nd, nt = _lib.LSE_MAX_DIMS, _lib.LSE_MAX_TERMS
        frame = tuple([3, 2, 5, 4, 3, 7][d % 6] for d in range(nd))
        terms = []
        for k in range(nt):                      # term k misses every dim d with (d + k) % 3 == 0
            terms.append(rnd(*[1 if (d + k) % 3 == 0 else frame[d] for d in range(nd)]))
        terms[-1].reshape(-1)[::5] = -INF
        return terms, frame, nd // 2
    if name == "strided":
        frame = (37, 65, 3)
        t0 = (rnd(65, 37, 3), "transpose01")                 # a transposed, non-contiguous view
        t1 = (rnd(1, 65, 1), ("expand", frame))              # stride 0
        t2 = rnd(37, 1, 3)
        t2.reshape(-1)[::4] = -INF
        return [t0, t1, t2], frame, 1
    if name == "cancel":
        frame = (257, 40)
        a, b, c = (torch.randn(257, 40, generator=g, dtype=F64) for _ in range(3))
        return [_round_to(1e4 + a, f32), _round_to(c, f32), _round_to(-1e4 + b, f32)], frame, 1
    for nm, frame, rdim, shapes in _lse_frames():
        if nm == name:
            terms = [rnd(*sh) for sh in shapes]
            terms[0].reshape(-1)[::7] = -INF                 # impossible assignments
            col = torch.zeros(frame[:rdim] + frame[rdim + 1:], dtype=F64)
            col.reshape(-1)[11] = -INF                       # a whole column: out = -inf, G = 0
            terms[0] += col.unsqueeze(rdim)
            return terms, frame, rdim
    raise ValueError(name)


def lse_view(term):
    """The tensor a term stands for: a recipe is applied to its base (on whichever device it is)."""
    if not isinstance(term, tuple):
        return term
    base, op = term
    return base.transpose(0, 1) if op == "transpose01" else base.expand(op[1])


def lse_reference(terms, frame, rdim, g_out, dtype=F64):
    """(out, G) in ``dtype``: torch.logsumexp of the summed terms and its autograd, G = 0 on an
    all -inf column."""
    total = torch.zeros(frame, dtype=dtype)
    for t in terms:
        total = total + t.to(dtype)
    total = total.detach().requires_grad_(True)
    out = torch.logsumexp(total, rdim)
    G, = torch.autograd.grad(out, total, g_out.to(dtype))
    G = torch.where((out == -INF).unsqueeze(rdim), torch.zeros_like(G), G)
    return out.detach(), G


@functools.lru_cache(maxsize=None)
def lse_case(name, f32):
    recipes, frame, rdim = lse_inputs(name, f32)
    terms = [lse_view(t) for t in recipes]
    kept = frame[:rdim] + frame[rdim + 1:]
    g = torch.Generator().manual_seed(len(name))
    g_out = _round_to(torch.randn(kept, generator=g, dtype=F64), f32)
    out, G = lse_reference(terms, frame, rdim, g_out)
    total = sum(t.expand(frame) for t in terms)
    mag = sum(torch.nan_to_num(t.expand(frame).abs(), posinf=0.0) for t in terms)
    arg = torch.nan_to_num(total, nan=-INF).argmax(rdim, keepdim=True)
    M = torch.gather(mag, rdim, arg).squeeze(rdim) + math.log(frame[rdim])
    c = {"terms": recipes, "frame": frame, "rdim": rdim, "g_out": g_out, "out": out.numpy(), "G": G.numpy(),
         "M": M.numpy(), "MG": (M * g_out.abs()).unsqueeze(rdim).numpy(), "cpu32": None}
    if f32:
        c["cpu32"] = tuple(x.double().numpy() for x in lse_reference(terms, frame, rdim, g_out, F32))
    return c


def lse_check(label, out, G, case, f32):
    c32 = case["cpu32"] or (None, None)
    check(label, "out", out, case["out"], case["M"], f32, c32[0])
    check(label, "G", G, case["G"], case["MG"], f32, c32[1])


# =======================================================================================================
# lda factor (pa_lda_factor_fwd_bwd, pa_lda_factor_indexed_fwd_bwd)
# =======================================================================================================
LDA_SEG = 2048
LDA_ROUTES = ("atomic", "indexed")
LDA_T = (1, 8, 9, 16, 17, 32, 33, 64)
KIB = 1024


def lda_tmax(T):
    return 8 if T <= 8 else 16 if T <= 16 else 32 if T <= 32 else 64


def lda_atomic_waves(V, tmax, esz):
    """lda_waves of csrc/lda.hip: two V x TMAX tables and NW x (TMAX + 1) x 64 values in 160 KiB."""
    for nw in (16, 8, 4, 2, 1):
        if 2 * V * tmax * esz + nw * (tmax + 1) * 64 * esz <= 160 * KIB:
            return nw, 160
    return 0, 0


def lda_indexed_waves(V, tmax, esz):
    """lda_doc_waves of csrc/lda.hip: one table; first under 64 KiB (two workgroups per CU), then 160."""
    for budget in (64, 160):
        for nw in (16, 8, 4, 2, 1):
            if V * tmax * esz + nw * (tmax + 1) * 64 * esz <= budget * KIB:
                return nw, budget
    return 0, 0


def lda_waves(route, V, tmax, esz):
    return (lda_atomic_waves if route == "atomic" else lda_indexed_waves)(V, tmax, esz)


def lda_cells(route, f32):
    """[(tmax, nw, tier KiB, V)]: for every reachable (TMAX, NW[, tier]) cell the largest V that lands
    in it, then (tmax, 0, 0, V) for the first V that no longer fits."""
    esz = 4 if f32 else 8
    ntab = 2 if route == "atomic" else 1
    cells = []
    for tmax in (8, 16, 32, 64):
        last = 0
        for budget in ((160,) if route == "atomic" else (64, 160)):
            for nw in (16, 8, 4, 2, 1):
                V = (budget * KIB - nw * (tmax + 1) * 64 * esz) // (ntab * tmax * esz)
                if V > last:                      # the cell is reachable: V in (last, V] lands in it
                    cells.append((tmax, nw, budget, V))
                    last = V
        cells.append((tmax, 0, 0, last + 1))
    return cells


_LDA_T_OF = {8: (1, 8), 16: (9, 16), 32: (17, 32), 64: (33, 64)}


def lda_cell_cases(route, f32):
    """[(T, V, B, Wd, tmax, nw, tier)] one launch per reachable cell; T alternates between the two
    values of LDA_T under the cell's TMAX, B between the ragged tiles 65 and 70."""
    out = []
    for i, (tmax, nw, tier, V) in enumerate(c for c in lda_cells(route, f32) if c[1]):
        out.append((_LDA_T_OF[tmax][i % 2], V, (65, 70)[(i // 2) % 2], 5, tmax, nw, tier))
    return out


def lda_refusals(route, f32):
    """[(T, V)] that the wrapper must refuse: the first V past every TMAX's last cell, and T = 65."""
    return [(_LDA_T_OF[c[0]][1], c[3]) for c in lda_cells(route, f32) if not c[1]] + [(65, 10)]


LDA_SIZES = [(B, Wd) for B in (1, 64, 65, 70) for Wd in (0, 1, 5)]
LDA_PATTERNS = ("absent_topic", "impossible_word", "impossible_doc", "shift1e3")
LDA_PATTERN_SHAPES = [(8, 50), (9, 50)]          # (T, V): a full TMAX and a padded one


def lda_inputs(T, V, B, Wd, f32, pattern=None, multi_segment=False):
    """(words int64 [Wd,B], lt [B,T], lp [T,V]) float64, representable in the target precision."""
    g = torch.Generator().manual_seed(T * 100003 + V * 101 + B * 7 + Wd)
    words = torch.randint(0, V, (Wd, B), generator=g)
    if multi_segment:                             # one word holds more than LDA_SEG pairs
        keep = torch.rand(Wd, B, generator=g) < 0.03
        words = torch.where(keep, words, torch.zeros_like(words))
    elif Wd:
        words[0, 0] = V - 1                       # the last row of the tables
        words[-1, -1] = 0
    lt = torch.log_softmax(2 * torch.randn(B, T, generator=g, dtype=F64), -1)
    lp = torch.log_softmax(3 * torch.randn(T, V, generator=g, dtype=F64), -1)
    d, v2 = B // 2, V - 2
    if pattern == "absent_topic":
        lt[d, T // 2] = -INF
        lt[0, 0] = -INF
    elif pattern == "impossible_word":
        lp[T // 2, words[0, d] if Wd else 0] = -INF
    elif pattern in ("impossible_doc", "impossible_doc_clean"):
        # word v2 occurs in document d only; d holds topic t2 alone, under which v2 is impossible
        words = torch.where(words == v2, torch.full_like(words, v2 - 1), words)
        words[0, d] = v2
        t2 = T - 1
        lt[d, :t2] = -INF
        lt[d, t2] = 0.0
        if pattern == "impossible_doc":
            lp[t2, v2] = -INF
    elif pattern == "shift1e3":
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).double()
        lt = lt + 1e3 * sign[:, None]
    elif pattern is not None:
        raise ValueError(pattern)
    return words, _round_to(lt, f32), _round_to(lp, f32)


def lda_reference(words, lt, lp, dtype=F64):
    """(out [B], g_theta [B,T], g_phi [T,V], M_out [B], M_gtheta [B,1], M_gphi [1,V]) in ``dtype``."""
    lt, lp = lt.to(dtype), lp.to(dtype)
    Wd, B = words.shape
    T, V = lp.shape
    s = lt.t()[:, None, :] + lp[:, words]                                 # [T, Wd, B]
    lse = torch.logsumexp(s, 0)                                           # [Wd, B]
    resp = torch.exp(s - lse[None])
    resp = torch.where((lse == -INF)[None], torch.zeros_like(resp), resp)
    out = lse.sum(0)
    g_theta = resp.sum(1).t().contiguous()
    g_phi = torch.zeros(T, V, dtype=dtype)
    g_phi.index_add_(1, words.reshape(-1), resp.reshape(T, -1))
    if Wd == 0:
        z = torch.zeros
        return out, g_theta, g_phi, z(B, dtype=F64), z(B, 1, dtype=F64), z(1, V, dtype=F64)
    top = torch.nan_to_num(s.double(), nan=-INF).argmax(0, keepdim=True)
    mag = torch.nan_to_num(lt.double().abs().t()[:, None, :] + lp.double().abs()[:, words], posinf=0.0)
    Mp = torch.gather(mag, 0, top)[0] + math.log(T)                       # [Wd, B] per pair
    Mv = torch.zeros(V, dtype=F64).index_add_(0, words.reshape(-1), Mp.reshape(-1))
    return out, g_theta, g_phi, Mp.sum(0), Mp.sum(0)[:, None], Mv[None, :]


@functools.lru_cache(maxsize=None)
def lda_case(T, V, B, Wd, f32, pattern=None, multi_segment=False):
    words, lt, lp = lda_inputs(T, V, B, Wd, f32, pattern, multi_segment)
    r = lda_reference(words, lt, lp)
    c = {"words": words, "lt": lt, "lp": lp, "ref": tuple(x.numpy() for x in r[:3]),
         "M": tuple(x.numpy() for x in r[3:]), "cpu32": None}
    if f32:
        c["cpu32"] = tuple(x.double().numpy() for x in lda_reference(words, lt, lp, F32)[:3])
    return c


def lda_check(label, got, case, f32):
    c32 = case["cpu32"] or (None, None, None)
    for what, g, r, M, c in zip(("out", "g_theta", "g_phi"), got, case["ref"], case["M"], c32):
        check(label, what, g, r, M, f32, c)
