"""Case grids, input builders, references, magnitudes and the tolerance rule of the many-small-sites kernels:
the ELBO assembly pa_multi_log_prob_sum / _grad / _sum_grad (csrc/multisite_dev.h), the mean-field draw
pa_meanfield_normal_sample with its backward, and the chained tail that runs them with Adam as phases of one
launch (csrc/chain.hip, csrc/site_tail.h).  test_multisite_edges_host.py runs the numpy restatements of
tests/oracle_backend.py against these references on the CPU, test_multisite_edges_gpu.py the HIP kernels.

References (float64 torch on the CPU, independent of the kernels and of oracle/):
  assembly  leaves value, p0, p1 in their own broadcast shapes ([R,C], [1,C], [R,1], [1,1]);
            total = coef_all sum_e coef_e sum(where(mask_e, log_prob_e, 0)), log_prob from
            dist_edge_cases.torch_log_prob (an identity entry, dist 100, is sum(value)); gradients by autograd of
            g * total.  Chained entries share the head's value leaf, so autograd gives the head the sum and the
            members nothing; the extra term is g coef_all extra_coef sum(extra_grad * value) added to the scalar.
  draw      eps against oracle.philox.normal; scale against float64 softplus (threshold 20);
            z = loc + scale * eps in float64 from the kernel's own eps.
  backward  autograd of sum(d_z (loc + softplus(rho) eps)) + sum(d_scale softplus(rho)) + sum(d_loc_out loc).
  tail      autograd of the step's scalar through z_k = loc_k + softplus(rho_k) eps_k with loc_out = loc and
            scale = softplus(rho) as the guide entry's parameters and eps_k as data, then one step of
            torch.optim.Adam(foreach=False) (ClippedAdam: guide_edge_cases.torch_clipped_adam_step, which the
            guide host test pins to the recorded reference) from a preset state.

Tolerance: the f32-class rule of tests/dist_edge_cases.py (``check`` is that module's):
  float64  the non-finite pattern is the reference's exactly; elsewhere |got - ref64| <= 64 eps64 M.
  float32  |got - ref64| <= 4 |cpu32 - ref64| + 8 eps32 M, cpu32 = the same torch formula in float32 on the CPU.
  M        per element dist_edge_cases.magnitude (times the absolute weight); a reduced output's M is the sum of
           its elements' M; the Adam outputs use guide_edge_cases.adam_magnitudes.
  Reduced outputs (the total, ROWRED / COLRED / SCALAR gradients, d_loc, d_rho): a thread adds k terms in the
  working type before the partial sums are combined in float64.  Each of those k - 1 float32 additions rounds a
  partial sum of magnitude at most M by at most eps32 / 2 (the unit round-off), so the float32 bound's last term
  becomes (8 + k / 2) eps32 M.  k is the largest number of terms one thread adds under the kernels' thread maps,
  restated below (grad_map, sum_map, bwd_map) and checked for self-consistency by the host test:
    combined_pass  tk = min(C, 256) threads along the columns, ng = min(8, 256 / tk) row groups; thread (c0, g)
                   owns rows g, g + ng, ... of columns c0, c0 + tk, ...: ROWRED k = ceil(R / ng) per column,
                   SCALAR k = ceil(R / ng) ceil(C / tk).
    operand_pass   (a reduced value operand, COLRED parameters) the same map on the kept dimension K and the summed
                   one L: k = ceil(L / ng); SCALAR: elements t, t + 256, ...: k = ceil(R C / 256).
    entry_sum      nth = 64 wpe threads (wpe = 16 / n waves per entry, 1 from 16 entries on), tk = min(C, nth),
                   ng = nth / tk: k = ceil(C / tk) ceil(R / ng).
    backward       tk = n below 256, 64 from n = 4096 on when P >= 16, else 256; ng as above; k = ceil(P / ng).
  Un-reduced outputs keep 8 eps32 M.  The geometry grids use ordinary inputs (values randn, scales and rates in
  [0.5, 2], positive-support values in [0.1, 3], counts small integers): nothing is unscored there (the host test
  asserts it).  The family-edge case inherits dist_edge_cases' grids and that module's rule as it stands: its
  grids hold points that overflow float32 on purpose (scales of 1e-30 beside values of 1e15), the float32 torch
  formula is non-finite on up to 27 % of an output there (Normal d_scale; Normal d_value 13 %, HalfNormal 14 / 25 %,
  KLscale 11 / 18 %, HalfCauchy 4 / 9 %, LogNormal 7 %, the other families 0), and dist_edge_cases asserts no cap on
  them: a 5 % cap cannot hold on those grids whatever the kernel does, so none is asserted for that case.

Found while writing these tests, and fixed:
  * entry_sum divides by tk = min(cols, nth); an entry with rows > 0, cols = 0 passed the host-side checks and
    reached that division in the total's workgroup.  multi_sum_partial now skips an entry with rows * cols == 0,
    as multi_grad_body always did.
  * The fused tail sums the entries that do not read the finalize phase's outputs before the wait and the others
    afterwards, selected by a bit mask in which 0 means "all": with no finalize phase recorded (or no entry reading
    its outputs) both calls summed every entry and the fused form returned TWICE the total of the separate launches
    (355.96 against 711.92 on the first table of case 8).  The second call is now made only for a non-empty mask.
  * Fam<Normal>::grad left d * d - 1 to the compiler's contraction, and whether it became one fma depended on the
    code around the inlined call: the separate launches formed the fma, the one-pass site code of site_tail.h
    rounded the product first, and the guide's d scale -- with it the gradient of rho and both Adam moments --
    differed in the last bit on 49 of 128 columns at (n, P) = (128, 16).  The step's parameters usually absorbed it,
    which is how tests/test_chain_gpu.py stayed green.  The fma is now spelled out (fam_fma), so every kernel that
    inlines the family rounds alike; the separate launches compute what they computed before.

Largest error / bound per kernel, path and dtype, measured on the MI355X by test_multisite_edges_gpu.py (1.0 would
be the bound):
  bwd/16sites/narrow/f32                 0.075    grad/degenerate/operand_rowred/f32     0.092
  bwd/16sites/narrow/f64                 0.029    grad/degenerate/operand_rowred/f64     0.026
  bwd/16sites/tile256/f32                0.107    grad/full/f32                          0.384
  bwd/16sites/tile256/f64                0.026    grad/full/f64                          0.050
  bwd/16sites/wide64/f32                 0.077    grad/odd/combined_rowred/f32           0.189
  bwd/16sites/wide64/f64                 0.023    grad/odd/combined_rowred/f64           0.045
  bwd/17sites/narrow/f32                 0.075    grad/odd/combined_scalar/f32           0.042
  bwd/17sites/narrow/f64                 0.029    grad/odd/combined_scalar/f64           0.005
  bwd/17sites/tile256/f32                0.107    grad/odd/full/f32                      0.250
  bwd/17sites/tile256/f64                0.026    grad/odd/full/f64                      0.031
  bwd/17sites/wide64/f32                 0.068    grad/odd/operand_colred/f32            0.050
  bwd/17sites/wide64/f64                 0.023    grad/odd/operand_colred/f64            0.011
  bwd/narrow/f32                         0.078    grad/odd/total/f32                     0.007
  bwd/narrow/f64                         0.026    grad/odd/total/f64                     0.000
  bwd/sinks/narrow/f32                   0.070    grad/operand_colred/f32                0.205
  bwd/sinks/narrow/f64                   0.015    grad/operand_colred/f64                0.078
  bwd/sinks/tile256/f32                  0.093    grad/operand_rowred/f32                0.215
  bwd/sinks/tile256/f64                  0.027    grad/operand_rowred/f64                0.079
  bwd/sinks/wide64/f32                   0.073    grad/operand_scalar/f32                0.095
  bwd/sinks/wide64/f64                   0.025    grad/operand_scalar/f64                0.034
  bwd/tile256/f32                        0.103    grad/total/f32                         0.008
  bwd/tile256/f64                        0.030    grad/total/f64                         0.008
  bwd/wide64/f32                         0.072    sum/alone/total/f32                    0.039
  bwd/wide64/f64                         0.030    sum/alone/total/f64                    0.014
  chain/combined_rowred/f32              0.140    sum/wpe1/total/f32                     0.004
  chain/combined_rowred/f64              0.032    sum/wpe1/total/f64                     0.003
  chain/combined_scalar/f32              0.058    sum/wpe16/total/f32                    0.019
  chain/combined_scalar/f64              0.015    sum/wpe16/total/f64                    0.000
  chain/full/f32                         0.266    sum/wpe2/total/f32                     0.001
  chain/full/f64                         0.046    sum/wpe2/total/f64                     0.002
  chain/operand_colred/f32               0.054    sum/wpe3/total/f32                     0.002
  chain/operand_colred/f64               0.024    sum/wpe3/total/f64                     0.000
  chain/total/f32                        0.026    sum/wpe4/total/f32                     0.006
  chain/total/f64                        0.007    sum/wpe4/total/f64                     0.004
  draw/block_generic/f32                 0.071    sum/wpe5/total/f32                     0.012
  draw/block_generic/f64                 0.015    sum/wpe5/total/f64                     0.008
  draw/block_vector/f32                  0.071    sum/wpe8/total/f32                     0.000
  draw/block_vector/f64                  0.016    sum/wpe8/total/f64                     0.006
  draw/element/f32                       0.057    sum_grad/wpe1/total/f32                0.001
  draw/element/f64                       0.000    sum_grad/wpe1/total/f64                0.012
  edges/chain/f32                        0.626    sum_grad/wpe16/total/f32               0.019
  edges/chain/f64                        0.910    sum_grad/wpe2/total/f32                0.001
  grad/combined_rowred/f32               0.230    sum_grad/wpe2/total/f64                0.006
  grad/combined_rowred/f64               0.072    sum_grad/wpe3/total/f32                0.002
  grad/combined_scalar/f32               0.090    sum_grad/wpe4/total/f32                0.006
  grad/combined_scalar/f64               0.062    sum_grad/wpe4/total/f64                0.011
  grad/degenerate/combined_rowred/f32    0.092    sum_grad/wpe5/total/f32                0.012
  grad/degenerate/combined_rowred/f64    0.026    sum_grad/wpe8/total/f32                0.000
  grad/degenerate/full/f32               0.265    tail/adam/f32                          0.239
  grad/degenerate/full/f64               0.039    tail/adam/f64                          0.028
  grad/degenerate/operand_colred/f32     0.086    tail/clipped/f32                       0.233
  grad/degenerate/operand_colred/f64     0.020    tail/clipped/f64                       0.032
"""
import functools
import math

import numpy as np
import torch

from tests import dist_edge_cases as ec
from tests import guide_edge_cases as gc
from tests.dist_edge_cases import EPS32, EPS64, F32_TINY, check  # noqa: F401

F32, F64 = torch.float32, torch.float64
INF = math.inf
UNSCORED_CAP = 0.05
RATIOS = {}                   # label -> largest error / bound seen by score() in this process
GRAD_THREADS, UN, MAX_ENTRIES, MF_MAX_SITES = 256, 8, 16, 16
IDENTITY = 100
TWO = ec.TWO_PARAM


def ratio_table():
    keys = sorted(RATIOS)
    half = (len(keys) + 1) // 2
    rows = []
    for i in range(half):
        row = "  %-38s %.3f" % (keys[i], RATIOS[keys[i]])
        if i + half < len(keys):
            row += "    %-38s %.3f" % (keys[i + half], RATIOS[keys[i + half]])
        rows.append(row)
    return "\n".join(rows)


def to32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def dt(f32):
    return F32 if f32 else F64


def dname(f32):
    return "f32" if f32 else "f64"


def cdiv(a, b):
    return -(-a // b)


# =======================================================================================================
# the rule
# =======================================================================================================

def unscored(ref64, cpu32):
    ref64, cpu32 = np.asarray(ref64, np.float64), np.asarray(cpu32, np.float64)
    return int((np.isfinite(ref64) & ~np.isfinite(cpu32)).sum())


def score(label, what, got, ref64, M, f32, cpu32=None, k=0, cap=0.0):
    """dist_edge_cases.check with the reduced-output amendment: in float32 the last term of the bound is
    (8 + k / 2) eps32 M (k = 0: an un-reduced output).  Records error / bound under ``label``.  ``cap``: the
    largest fraction of elements the float32 comparison may leave unscored."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, "%s %s: shape %s, reference %s" % (label, what, got.shape, ref64.shape)
    M = np.broadcast_to(np.asarray(M, np.float64), got.shape)
    Meff = M * ((8 + k / 2) / 8) if f32 else M
    with np.errstate(all="ignore"):
        if f32:
            cpu32 = np.broadcast_to(np.asarray(cpu32, np.float64), got.shape)
            if got.size:
                assert unscored(ref64, cpu32) <= cap * got.size, "%s %s: %d of %d elements unscored" % (
                    label, what, unscored(ref64, cpu32), got.size)
            bound = 4 * np.abs(cpu32 - ref64) + 8 * EPS32 * Meff + F32_TINY
            scored = np.isfinite(cpu32) & np.isfinite(ref64) & np.isfinite(got)
        else:
            bound = 64 * EPS64 * Meff
            scored = np.isfinite(ref64) & np.isfinite(got)
        err = np.where(got == ref64, 0.0, np.abs(got - ref64))
        ratio = np.where(scored, err / np.where(bound > 0, bound, 1.0), 0.0)
        ratio = np.where(scored & (bound == 0) & (err > 0), np.inf, ratio)
    if ratio.size:
        RATIOS[label] = max(RATIOS.get(label, 0.0), float(ratio.max()))
    check("%s %s" % (label, what), got, ref64, Meff, f32, cpu32)


# =======================================================================================================
# the thread maps, restated
# =======================================================================================================
PATTERNS = {"F": "full", "R": "rowred", "C": "colred", "S": "scalar"}


def op_shape(p, R, C):
    return {"F": (R, C), "R": (1, C), "C": (R, 1), "S": (1, 1)}[p]


def pattern_of(shape, R, C):
    """pattern_of of the kernel: a stride-0 dimension of extent 1 is not a reduction."""
    red_r, red_c = shape[0] == 1 and R > 1, shape[1] == 1 and C > 1
    return ("scalar" if red_c else "rowred") if red_r else ("colred" if red_c else "full")


def grad_map(K):
    """(tk, ng) of combined_pass / operand_pass / the backward for K kept indices."""
    tk = min(K, GRAD_THREADS)
    return tk, min(8, GRAD_THREADS // tk)


def k_grad(R, C, which, pat):
    """Terms one thread adds for operand ``which`` (0 value, 1 p0, 2 p1) with pattern ``pat``; 0 = un-reduced."""
    if pat == "full":
        return 0
    generic = which == 0 or pat == "colred"           # operand_pass
    if pat == "scalar":
        if generic:
            return cdiv(R * C, GRAD_THREADS)
        tk, ng = grad_map(C)
        return cdiv(R, ng) * cdiv(C, tk)
    K, L = (C, R) if pat == "rowred" else (R, C)
    tk, ng = grad_map(K)
    return cdiv(L, ng)


def grad_path(which, pat):
    if pat == "full":
        return "full"
    return ("operand_" if (which == 0 or pat == "colred") else "combined_") + pat


def sum_map(C, n_entries, waves=16):
    """(wpe, tk, ng) of entry_sum for an entry of C columns in a table of n_entries."""
    wpe = 1 if n_entries >= waves else waves // max(n_entries, 1)
    nth = 64 * wpe
    tk = min(C, nth)
    return wpe, tk, nth // tk


def k_sum(R, C, n_entries, waves=16):
    if R * C == 0:
        return 0
    _, tk, ng = sum_map(C, n_entries, waves)
    return cdiv(C, tk) * cdiv(R, ng)


def bwd_map(n, P):
    tk = n if n < 256 else (64 if (n >= 4096 and P >= 16) else 256)
    return tk, min(8, GRAD_THREADS // tk)


def bwd_path(n, P):
    return "narrow" if n < 256 else ("wide64" if (n >= 4096 and P >= 16) else "tile256")


def k_bwd(n, P):
    return cdiv(P, bwd_map(n, P)[1])


def thread_elements(R, C):
    """combined_pass's element -> thread map by brute force: owner[r, c] = thread, following the kernel's loops
    (column blocks of tk, rows in batches of UN * ng).  The host test checks it against grad_map / k_grad."""
    tk, ng = grad_map(C)
    owner = np.full((R, C), -1, np.int64)
    for t in range(GRAD_THREADS):
        c0, g = t % tk, t // tk
        for cb in range(0, C, tk):
            c = cb + c0
            if not (g < ng and c < C):
                continue
            for rb in range(g, R, UN * ng):
                for u in range(UN):
                    r = rb + u * ng
                    if r < R:
                        assert owner[r, c] == -1
                        owner[r, c] = t
    return owner


def sum_elements(R, C, n_entries):
    """entry_sum's element -> thread map by brute force (UNS = 4)."""
    wpe, tk, ng = sum_map(C, n_entries)
    owner = np.full((R, C), -1, np.int64)
    for t in range(64 * wpe):
        c0, g = t % tk, t // tk
        if g >= ng:
            continue
        for c in range(c0, C, tk):
            for rb in range(g, R, 4 * ng):
                for u in range(4):
                    r = rb + u * ng
                    if r < R:
                        assert owner[r, c] == -1
                        owner[r, c] = t
    return owner


# =======================================================================================================
# assembly: entries, reference, magnitudes
# =======================================================================================================
# operand kinds per family (value, p0, p1): n randn, s in [0.5, 2], p in [0.1, 3], u in [0.1, 0.9], b 0 / 1,
# c counts 0..4, N counts 5..8
KINDS = {0: "nns", 1: "bn-", 2: "ps-", 3: "pns", 4: "ps-", 5: "ps-", 6: "pss", 7: "uss", 8: "cs-", 9: "cnN",
         10: "nns", 11: "ss-", IDENTITY: "n--"}
VALUE_GRAD = "nspu"           # value kinds a value gradient is asked for


def draw(rng, kind, shape):
    if kind == "n":
        x = rng.standard_normal(shape)
    elif kind == "s":
        x = rng.uniform(0.5, 2.0, shape)
    elif kind == "p":
        x = rng.uniform(0.1, 3.0, shape)
    elif kind == "u":
        x = rng.uniform(0.1, 0.9, shape)
    elif kind == "b":
        x = (rng.uniform(size=shape) < 0.4) * 1.0
    elif kind == "c":
        x = rng.integers(0, 5, shape) * 1.0
    elif kind == "N":
        x = rng.integers(5, 9, shape) * 1.0
    else:
        raise ValueError(kind)
    return torch.tensor(to32(x), dtype=F64).reshape(shape)


def make_mask(rng, p, R, C):
    if p is None:
        return None
    return torch.tensor(rng.uniform(size=op_shape(p, R, C)) < 0.7)


def entry(rng, dist, R, C, pats="FFF", mask=None, coef=1.0, need=None, value=None, **kw):
    """One table entry on CPU float64 tensors, in the dict format of kernels.multi_log_prob_grad."""
    kinds = KINDS[dist]
    ops = []
    for j in range(3):
        ops.append(None if kinds[j] == "-" else draw(rng, kinds[j], op_shape(pats[j], R, C)))
    if value is not None:
        ops[0] = value
    if need is None:
        need = (kinds[0] in VALUE_GRAD, kinds[1] != "-", kinds[2] != "-")
    e = dict(dist=dist, rows=R, cols=C, value=ops[0], p0=ops[1], p1=ops[2], mask=make_mask(rng, mask, R, C),
             coef=coef, need=tuple(need))
    e.update(kw)
    return e


def heads_of(entries):
    """index of the chain head whose value leaf entry i scores (itself unless by_chain)."""
    head = list(range(len(entries)))
    for i, e in enumerate(entries):
        if e.get("by_chain"):
            continue
        k = e.get("chain_next", -1)
        while k >= 0:
            head[k] = i
            k = entries[k].get("chain_next", -1)
    return head


def log_prob(dist, v, a, b):
    return v if dist == IDENTITY else ec.torch_log_prob(dist, v, a, b)


def assembly(entries, coef_all, g, dtype):
    """(total, [(dv, da, db)]) float64 numpy: torch in ``dtype``, gradients by autograd of g * total (+ extras),
    each in its operand's own broadcast shape (None where the entry has no such operand / asks for none)."""
    head = heads_of(entries)
    leaves = [[None if e[key] is None else e[key].detach().to(dtype).clone().requires_grad_(True)
               for key in ("value", "p0", "p1")] for e in entries]
    total = torch.zeros((), dtype=dtype)
    extra = torch.zeros((), dtype=dtype)
    for i, e in enumerate(entries):
        R, C = e["rows"], e["cols"]
        if R * C == 0 or e["dist"] == 101:
            continue
        v = leaves[head[i]][0].expand(R, C)
        a, b = (None if x is None else x.expand(R, C) for x in leaves[i][1:])
        lp = log_prob(e["dist"], v, a, b)
        if e["mask"] is not None:
            lp = torch.where(e["mask"].expand(R, C), lp, torch.zeros((), dtype=dtype))
        total = total + e["coef"] * lp.sum()
        if e.get("extra_grad") is not None:
            extra = extra + e["extra_coef"] * (e["extra_grad"].to(dtype).reshape(R, C) * v).sum()
    total = coef_all * total
    scalar = g * (total + coef_all * extra)
    flat = [x for row in leaves for x in row if x is not None]
    gs = iter(torch.autograd.grad(scalar, flat, allow_unused=True) if scalar.requires_grad else [None] * len(flat))
    grads = []
    for i, (e, row) in enumerate(zip(entries, leaves)):
        out = []
        for j, x in enumerate(row):
            gx = None if x is None else next(gs)
            want = x is not None and e["need"][j] and not (j == 0 and e.get("by_chain"))
            if want and gx is None:
                gx = torch.zeros_like(x)
            out.append(gx.double().numpy() if want else None)
        grads.append(tuple(out))
    return float(total.detach().double()), grads


def _elem_magnitude(e, v):
    R, C = e["rows"], e["cols"]
    bc = lambda t: np.zeros((R, C)) if t is None else np.broadcast_to(t.numpy(), (R, C)).astype(np.float64)  # noqa: E731
    v = bc(v)
    if e["dist"] == IDENTITY:
        M = {"lp": np.abs(v), "dv": np.ones((R, C)), "da": np.zeros((R, C)), "db": np.zeros((R, C))}
    else:
        M = ec.magnitude(e["dist"], v, bc(e["p0"]), bc(e["p1"]))
        M = {k_: np.broadcast_to(np.nan_to_num(x, nan=0.0, posinf=0.0), (R, C)) for k_, x in M.items()}
    if e["mask"] is not None:
        m = np.broadcast_to(e["mask"].numpy(), (R, C))
        M = {k_: np.where(m, x, 0.0) for k_, x in M.items()}
    return M


def _reduce_to(x, shape):
    if shape[0] == 1 and x.shape[0] > 1:
        x = x.sum(0, keepdims=True)
    if shape[1] == 1 and x.shape[1] > 1:
        x = x.sum(1, keepdims=True)
    return x


def assembly_magnitudes(entries, coef_all, g):
    """(M of the total, [(Mv, Ma, Mb)] in the operands' own shapes, [M of entry e's own share of the total])."""
    head = heads_of(entries)
    per = []
    for i, e in enumerate(entries):
        per.append(None if e["rows"] * e["cols"] == 0 or e["dist"] == 101
                   else _elem_magnitude(e, entries[head[i]]["value"]))
    shares = [0.0 if M is None else abs(coef_all * e["coef"]) * float(M["lp"].sum()) for e, M in zip(entries, per)]
    out = []
    for i, (e, M) in enumerate(zip(entries, per)):
        if M is None:
            out.append((None, None, None))
            continue
        w = abs(g * coef_all * e["coef"])
        Mv = w * M["dv"]
        k = e.get("chain_next", -1) if not e.get("by_chain") else -1
        while k >= 0:
            Mv = Mv + abs(g * coef_all * entries[k]["coef"]) * per[k]["dv"]
            k = entries[k].get("chain_next", -1)
        if e.get("extra_grad") is not None:
            Mv = Mv + abs(g * coef_all * e["extra_coef"]) * np.abs(e["extra_grad"].numpy().reshape(Mv.shape))
        row = []
        for key, Mx in zip(("value", "p0", "p1"), (Mv, w * M["da"], w * M["db"])):
            row.append(None if e[key] is None else _reduce_to(Mx, tuple(e[key].shape)))
        out.append(tuple(row))
    return float(sum(shares)), out, shares


def assembly_case(entries, coef_all, g, f32):
    """Everything score() needs for one table: ref, cpu32 (float32 cases), M, and k per output."""
    with np.errstate(all="ignore"):
        ref = assembly(entries, coef_all, g, F64)
        cpu32 = assembly(entries, coef_all, g, F32) if f32 else None
        M = assembly_magnitudes(entries, coef_all, g)
    n = len(entries)
    ks, paths = [], []
    for e in entries:
        R, C = e["rows"], e["cols"]
        pats = [None if e[key] is None else pattern_of(tuple(e[key].shape), R, C) for key in ("value", "p0", "p1")]
        ks.append(tuple(0 if p is None else k_grad(R, C, j, p) for j, p in enumerate(pats)))
        paths.append(tuple(None if p is None else grad_path(j, p) for j, p in enumerate(pats)))
    k_tot = max([k_sum(e["rows"], e["cols"], min(n, MAX_ENTRIES)) for e in entries] + [0])
    return dict(entries=entries, coef_all=coef_all, g=g, ref=ref, cpu32=cpu32, M=M, k=ks, paths=paths, k_total=k_tot)


def score_assembly(label, case, f32, total=None, grads=None, cap=0.0, path_labels=True):
    """The rule on a table's outputs: ``total`` a float, ``grads`` [(dv, da, db)] numpy arrays / None."""
    name = dname(f32)
    if total is not None:
        c32 = None if case["cpu32"] is None else case["cpu32"][0]
        score("%s/total/%s" % (label, name), "total", np.float64(total), case["ref"][0], case["M"][0], f32, c32,
              k=case["k_total"], cap=cap)
    if grads is None:
        return
    assert len(grads) == len(case["entries"])
    for i, (e, got, ref, M, ks, paths) in enumerate(zip(case["entries"], grads, case["ref"][1], case["M"][1],
                                                        case["k"], case["paths"])):
        c32 = (None, None, None) if case["cpu32"] is None else case["cpu32"][1][i]
        for j, what in enumerate(("d_value", "d_p0", "d_p1")):
            assert (got[j] is None) == (ref[j] is None), "%s entry %d %s: produced %s, reference %s" % (
                label, i, what, got[j] is not None, ref[j] is not None)
            if ref[j] is None:
                continue
            lab = "%s/%s/%s" % (label, paths[j], name) if path_labels else "%s/grad/%s" % (label, name)
            score(lab, "entry %d (dist %d, %dx%d) %s" % (i, e["dist"], e["rows"], e["cols"], what),
                  np.asarray(got[j], np.float64).reshape(ref[j].shape), ref[j], M[j], f32, c32[j], k=ks[j], cap=cap)


# ---- case 1: the thread map of the gradient pass -----------------------------------------------------
THREAD_MAP_C = (1, 32, 33, 64, 65, 128, 129, 256, 257, 513)


def thread_map_rows(C):
    ng = grad_map(C)[1]
    return sorted({1, ng, ng + 1, 8 * ng, 8 * ng + 1})


@functools.lru_cache(maxsize=None)
def thread_map_table(C):
    """One table per C: every R of the grid with every operand FULL, and again with p0 ROWRED and p1 SCALAR."""
    rng = np.random.default_rng(1000 + C)
    ents = []
    for R in thread_map_rows(C):
        for pats in ("FFF", "FRS"):
            ents.append(entry(rng, 0, R, C, pats, coef=(-1.5 if R % 2 else 0.75)))
    return ents


# ---- case 2: operand patterns ---------------------------------------------------------------------------
PATTERN_FRAMES = ((9, 33), (17, 129), (3, 257))
DEGENERATE_FRAMES = ((1, 33), (9, 1), (1, 1))
MASKS = (None, "F", "R", "C")


def _chunks(ents, n=MAX_ENTRIES):
    return [ents[i:i + n] for i in range(0, len(ents), n)]


@functools.lru_cache(maxsize=None)
def pattern_tables(R, C, masked=True):
    """All 4^3 operand patterns of a Normal entry (x the four mask shapes) on one frame, 16 entries a table."""
    rng = np.random.default_rng(2000 + 7 * R + C)
    ents = []
    for m in (MASKS if masked else (None,)):
        for pv in "FRCS":
            for pa in "FRCS":
                for pb in "FRCS":
                    ents.append(entry(rng, 0, R, C, pv + pa + pb, mask=m, coef=rng.choice([-2.0, 0.5, 1.25])))
    return _chunks(ents)


@functools.lru_cache(maxsize=None)
def odd_entries_table():
    """Non-contiguous values (a transposed view, a column slice), the one-parameter families with ``need`` set
    for p1 (``force_p1``: an output buffer is handed over and must stay untouched), an identity entry, an entry
    that asks for nothing, and empty entries [0, 4] and [4, 0]."""
    rng = np.random.default_rng(2999)
    R, C = 9, 33
    ents = []
    base = draw(rng, "n", (C, R))
    ents.append(entry(rng, 0, R, C, "FRC", value=base.t(), coef=-0.5))
    wide = draw(rng, "n", (R, 2 * C + 3))
    ents.append(entry(rng, 0, R, C, "FFS", value=wide[:, 2:2 + 2 * C:2], mask="F", coef=1.5))
    for d in (1, 2, 4, 5, 8, 11):
        ents.append(entry(rng, d, R, C, "FR-", coef=0.75, force_p1=True))
    ents.append(entry(rng, IDENTITY, 1, 64, coef=-1.25))
    ents.append(entry(rng, IDENTITY, R, C, mask="R", coef=2.0))
    ents.append(entry(rng, 6, R, C, "FCR", need=(False, False, False), coef=1.0))
    for shape in ((0, 4), (4, 0)):
        z = torch.zeros(shape, dtype=F64)
        ents.append(dict(dist=0, rows=shape[0], cols=shape[1], value=z, p0=z.clone(), p1=z.clone() + 1, mask=None,
                         coef=1.0, need=(True, True, True)))
    assert len(ents) <= MAX_ENTRIES
    return ents


# ---- case 3: the total ------------------------------------------------------------------------------------
TOTAL_N = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)
_TOTAL_FAMILIES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, IDENTITY)


@functools.lru_cache(maxsize=None)
def total_table(n):
    """n entries of cycling families with signed coefficients: C below, at and above the 64 wpe threads an entry
    gets (and a narrow C = 7), R at 4 ng - 1, 4 ng, 4 ng + 1 (the batches of UNS = 4 rows per group); every
    third entry masked."""
    rng = np.random.default_rng(3000 + n)
    nth = 64 * sum_map(1, min(n, MAX_ENTRIES))[0]
    ents = []
    for i in range(n):
        C = (nth - 1, nth, nth + 1, 7)[i % 4]
        ng = sum_map(C, min(n, MAX_ENTRIES))[2]
        R = max(1, 4 * ng + (-1, 1, 0)[(i // 4) % 3])
        ents.append(entry(rng, _TOTAL_FAMILIES[i % len(_TOTAL_FAMILIES)], R, C, "FFF"[:3],
                          mask=("F", None, None)[i % 3], coef=(-1.0) ** i * (0.5 + (i % 3)),
                          need=(False, False, False)))
        assert R * C <= 65536
    return ents


# ---- case 4: chains and extras ----------------------------------------------------------------------------
def _member(rng, dist, R, C, pats, coef, nxt=-1):
    e = entry(rng, dist, R, C, "F" + pats, coef=coef, chain_next=nxt, by_chain=True)
    e["value"] = None                                    # filled in by _link: the head's tensor
    return e


def _link(ents):
    head = heads_of(ents)
    for i, e in enumerate(ents):
        if e.get("by_chain"):
            e["value"] = ents[head[i]]["value"]
            e["need"] = (True,) + tuple(e["need"][1:])
    return ents


CHAIN_MEMBERS = (3, 2, 0)                  # LogNormal, HalfCauchy, Normal chained on a Gamma head's positive value


@functools.lru_cache(maxsize=None)
def chain_table(members, frame, xcoef, seed=0):
    """A Gamma head with ``members`` chained entries of different families, the members' parameters in rotating
    patterns, and the extra term (extra_coef ``xcoef``; None: no extra term)."""
    R, C = frame
    rng = np.random.default_rng(4000 + 100 * members + R + seed)
    pats = ("RS", "CF", "SC", "FR")
    ents = [entry(rng, 6, R, C, "F" + pats[(seed + 3) % 4], coef=-1.0, chain_next=1 if members else -1)]
    for q in range(members):
        ents.append(_member(rng, CHAIN_MEMBERS[q], R, C, pats[(q + seed) % 4], (0.5, -1.5, 2.0)[q],
                            q + 2 if q + 1 < members else -1))
    if xcoef is not None:
        ents[0]["extra_grad"] = draw(rng, "n", (R, C))
        ents[0]["extra_coef"] = xcoef
    return _link(ents)


@functools.lru_cache(maxsize=None)
def two_chains_table():
    """Two independent chains in one table, neither head at entry 0, one chain pointing backwards:
    [member of B, head B, a plain entry, head A, member A1, member A2]."""
    rng = np.random.default_rng(4500)
    RA, CA, RB, CB = 17, 129, 9, 33
    ents = [_member(rng, 0, RB, CB, "RS", 0.5),
            entry(rng, 3, RB, CB, "FSR", coef=-1.0, chain_next=0),
            entry(rng, 0, 5, 40, "FRC", mask="F", coef=1.5),
            entry(rng, 6, RA, CA, "FCR", coef=2.0, chain_next=4),
            _member(rng, 2, RA, CA, "F-", -0.5, 5),
            _member(rng, 0, RA, CA, "CR", 1.0)]
    ents[3]["extra_grad"], ents[3]["extra_coef"] = draw(rng, "n", (RA, CA)), -2.0
    return _link(ents)


def refusal_tables():
    """[(why, entries)]: tables the host refuses before any launch."""
    rng = np.random.default_rng(4600)
    out = []
    ents = [entry(rng, 0, 9, 33, "RFF", chain_next=1), _member(rng, 0, 9, 33, "RS", 1.0)]
    ents[1]["value"] = ents[0]["value"]
    out.append(("a chain on a broadcast value", ents))
    ents = [entry(rng, 0, 9, 33, "FFF", chain_next=1), _member(rng, 0, 9, 32, "RS", 1.0)]
    ents[1]["value"] = draw(rng, "n", (9, 32))
    out.append(("a frame mismatch", ents))
    out.append(("chain_next == k", [entry(rng, 0, 9, 33, "FFF", chain_next=0)]))
    return out


# ---- case 5: the families at the edges, through chains ---------------------------------------------------
def edge_chain_case(dist, f32, rng):
    """dist's edge grid on a [2, n] frame as a chain head (masked), a Normal(0.5, 2) member chained on it.
    -> dict: entries, w = (head, member) weights with coef_all = 2, ref / cpu32 / M of the head's d_value, d_p0,
    d_p1 and of the member's d_p0 / d_p1 per element (float64 numpy; reductions are done by the caller)."""
    v, a, b = ec.grid(dist, f32)
    n = v.size
    two = dist in TWO
    st = lambda x: torch.tensor(np.stack([x, x]), dtype=F64)   # noqa: E731
    m = rng.uniform(size=(2, n)) < 0.7
    m[:, 0] = True
    coef = (0.5, 2.0, 1.0, 0.25)[dist % 4]
    head = dict(dist=dist, rows=2, cols=n, value=st(v), p0=st(a), p1=st(b) if two else None, mask=torch.tensor(m),
                coef=coef, need=(True, True, two), chain_next=1)
    mem = dict(dist=0, rows=2, cols=n, value=head["value"], p0=torch.full((1, 1), 0.5, dtype=F64),
               p1=torch.full((1, 1), 2.0, dtype=F64), mask=None, coef=-0.5, need=(True, False, False), by_chain=True,
               chain_next=-1)
    wh, wm = 2.0 * coef, 2.0 * -0.5
    out = {"entries": [head, mem], "n": n}
    with np.errstate(all="ignore"):
        for name, dtype in (("ref", F64), ("cpu32", F32)):
            if dtype == F32 and not f32:
                out[name] = None
                continue
            rh = ec.reference(dist, v, a, b, dtype)
            rn = ec.reference(0, v, np.full(n, 0.5), np.full(n, 2.0), dtype)
            f = lambda x: np.where(m, wh * np.stack([x, x]), 0.0)   # noqa: E731
            dv = f(rh["dv"]) + wm * np.stack([rn["dv"], rn["dv"]])
            if dtype == F32:
                dv = to32(dv)
            out[name] = (dv, f(rh["da"]), f(rh["db"]) if two else None)
        Mh = ec.magnitude(dist, v, a, b)
        Mn = ec.magnitude(0, v, np.full(n, 0.5), np.full(n, 2.0))
        g = lambda x: np.nan_to_num(np.where(m, abs(wh) * np.stack([x, x]), 0.0), nan=0.0, posinf=0.0)   # noqa: E731
        out["M"] = (g(Mh["dv"]) + np.nan_to_num(abs(wm) * np.stack([Mn["dv"], Mn["dv"]]), nan=0.0, posinf=0.0),
                    g(Mh["da"]), g(Mh["db"]) if two else None)
    return out


# =======================================================================================================
# the draw and its backward
# =======================================================================================================
DRAW_RHO = (-104.0, -88.0, -20.0, 0.0, 19.999, 20.0, 20.001, 80.0)
DRAW_LOC = (0.0, 1e4, -1e4, 1e-30)
DRAW_N = (1, 3, 4, 5)
DRAW_P = (1, 2, 5)
BWD_N = (1, 2, 32, 33, 255, 256, 257, 4095, 4096, 4097)
BWD_RHO = (19.999, 20.0, 20.001, -3.0, 0.5, 25.0)


def draw_params(n, f32, shift=0):
    """(loc, rho) float64 numpy, n elements cycling through DRAW_LOC x DRAW_RHO (every pair within 32 elements)."""
    i = np.arange(n) + shift
    loc = np.array(DRAW_LOC)[i % 4]
    rho = np.array(DRAW_RHO)[(i // 4) % 8]
    return to32(loc), to32(rho)


def softplus(rho, dtype):
    return torch.nn.functional.softplus(torch.as_tensor(rho, dtype=dtype), threshold=20).double().numpy()


def draw_reference(loc, rho, eps, dtype):
    """(z, scale) float64 numpy from the kernel's own eps [P, n]."""
    with np.errstate(all="ignore"):
        sc = torch.nn.functional.softplus(torch.as_tensor(rho, dtype=dtype), threshold=20)
        z = torch.as_tensor(loc, dtype=dtype) + sc * torch.as_tensor(eps, dtype=dtype)
    return z.double().numpy(), sc.double().numpy()


def draw_magnitudes(loc, rho, eps):
    sc = softplus(rho, F64)
    return np.abs(loc)[None, :] + sc[None, :] * np.abs(eps), np.abs(sc) + 1.0       # (log1p(exp x): exp x + 1)


def bwd_P(n):
    ng = bwd_map(n, 1)[1]
    return sorted({1, 8 * ng - 1, 8 * ng, 8 * ng + 1, 15, 16})


def bwd_inputs(n, P, seed=0):
    """rho (around 20 and ordinary), eps, d_z [P, n], d_scale, d_loc_out [n]: float64 numpy, float32-exact."""
    rng = np.random.default_rng(7000 + 31 * n + P + seed)
    rho = to32(np.array(BWD_RHO)[(np.arange(n) + seed) % len(BWD_RHO)])
    return dict(rho=rho, eps=to32(rng.standard_normal((P, n))), d_z=to32(rng.standard_normal((P, n))),
                d_scale=to32(rng.standard_normal(n)), d_loc_out=to32(rng.standard_normal(n)))


def bwd_reference(inp, which, dtype):
    """(d_loc, d_rho) float64 numpy by autograd; ``which`` = (d_z, d_scale, d_loc_out) present."""
    t = lambda x: torch.as_tensor(x, dtype=dtype)   # noqa: E731
    n = inp["rho"].size
    loc = torch.zeros(n, dtype=dtype, requires_grad=True)
    rho = t(inp["rho"]).clone().requires_grad_(True)
    sp = torch.nn.functional.softplus(rho, threshold=20)
    s = (loc * 0).sum() + (rho * 0).sum()
    if which[0]:
        s = s + (t(inp["d_z"]) * (loc + sp * t(inp["eps"]))).sum()
    if which[1]:
        s = s + (t(inp["d_scale"]) * sp).sum()
    if which[2]:
        s = s + (t(inp["d_loc_out"]) * loc).sum()
    gl, gr = torch.autograd.grad(s, (loc, rho))
    return gl.double().numpy(), gr.double().numpy()


def bwd_magnitudes(inp, which):
    sig = np.where(inp["rho"] > 20, 1.0, 1.0 / (1.0 + np.exp(-inp["rho"])))
    Ml = np.zeros_like(inp["rho"])
    Mr = np.zeros_like(inp["rho"])
    if which[0]:
        Ml = Ml + np.abs(inp["d_z"]).sum(0)
        Mr = Mr + np.abs(inp["d_z"] * inp["eps"]).sum(0)
    if which[1]:
        Mr = Mr + np.abs(inp["d_scale"])
    if which[2]:
        Ml = Ml + np.abs(inp["d_loc_out"])
    return Ml, Mr * sig


@functools.lru_cache(maxsize=None)
def bwd_case(n, P, which, f32, seed=0):
    inp = bwd_inputs(n, P, seed)
    return dict(inp=inp, ref=bwd_reference(inp, which, F64), cpu32=bwd_reference(inp, which, F32) if f32 else None,
                M=bwd_magnitudes(inp, which), k=k_bwd(n, P) + 1, path=bwd_path(n, P))


def score_bwd(label, got, case, f32, add=0.0):
    """The rule on (d_loc, d_rho); ``add``: what an accumulating sink held before (it joins ref, cpu32 and M)."""
    c32 = case["cpu32"] or (None, None)
    for what, g, r, M, c in zip(("d_loc", "d_rho"), got, case["ref"], case["M"], c32):
        score("%s/%s/%s" % (label, case["path"], dname(f32)), what, g, r + add, M + abs(add), f32,
              None if c is None else to32(c + add), k=case["k"])


WHICH = tuple((a, b, c) for a in (True, False) for b in (True, False) for c in (True, False))


# =======================================================================================================
# the whole tail
# =======================================================================================================
FAST_COLS_ELIGIBLE = ((2, 64), (32, 64), (33, 56), (128, 16), (129, 8), (256, 8))
FAST_COLS_FALLBACK = ((32, 65), (33, 57), (129, 9), (257, 8))
FAST_SCALAR_ELIGIBLE = (2, 63, 64)
FAST_SCALAR_FALLBACK = (1, 65)
TAIL_HYPER = {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8, "wd": 0.1, "clip": 0.5, "lrd": 0.99}
TAIL_STEP0 = 7


def fast_site_expected(n, P, prior=0, masked=False):
    """The eligibility rule of the one-pass site code, restated: a Normal prior head, nothing masked, and
    COLS: 2 <= n <= 256 with P <= 8 min(8, 256 / n); SCALAR (n = 1, frame [1, P]): 2 <= P <= 64."""
    if prior != 0 or masked:
        return False
    if n == 1:
        return 2 <= P <= 64
    return 2 <= n <= 256 and P <= UN * min(8, GRAD_THREADS // n)


def tail_sites(shapes, P, seed, priors=None, masked=None):
    """Per site: n, prior family, its parameters, whether the head is masked: [(n, prior, p0, p1, mask or None)].
    A scalar site (n = 1) scores z on the frame [1, P], every other on [P, n]."""
    rng = np.random.default_rng(8000 + seed)
    out = []
    for i, n in enumerate(shapes):
        prior = 0 if priors is None else priors[i]
        frame = (1, P) if n == 1 else (P, n)
        p0 = draw(rng, "s" if prior == 6 else "n", (1, 1))
        p1 = draw(rng, "s", (1, 1))
        m = make_mask(rng, "F", *frame) if (masked is not None and masked[i]) else None
        out.append((n, prior, p0, p1, m))
    return out


def tail_inputs(sites, P, clipped, seed):
    """The flat parameter buffer [locs..., rhos...] with its optimizer state and the extra gradients."""
    rng = np.random.default_rng(8100 + seed)
    N = 2 * sum(s[0] for s in sites)
    p = rng.standard_normal(N) * 0.3
    off, locs, rhos = 0, [], []
    for s in sites:
        locs.append((off, s[0]))
        off += s[0]
    for s in sites:
        rhos.append((off, s[0]))
        off += s[0]
    for (o, n), s in zip(locs, sites):
        if s[1] == 6:
            p[o:o + n] = 2.0 + 0.1 * rng.standard_normal(n)           # a Gamma prior scores positive draws
    for (o, n), s in zip(rhos, sites):
        p[o:o + n] = rng.uniform(-3.0, -1.0, n)                        # scales of 0.05 .. 0.3
    return dict(p=to32(p), g=to32(0.1 * rng.standard_normal(N)), m=to32(0.05 * rng.standard_normal(N)),
                v=to32((0.1 * rng.standard_normal(N)) ** 2 + 1e-4), locs=locs, rhos=rhos,
                extra=[to32(rng.standard_normal((P, s[0]))) for s in sites])


def _tail_site_terms(s, loc, sc, z, P, t, dtype):
    """log p(z) (masked) and log q(z) of one site on the frame [P, n] (a scalar site's [1, P] is the same memory)."""
    n, prior, p0, p1, m = s
    lp = ec.torch_log_prob(prior, z, t(p0).expand(P, n), t(p1).expand(P, n))
    if m is not None:
        lp = torch.where(m.reshape(P, n), lp, torch.zeros((), dtype=dtype))
    return lp.sum(), ec.torch_log_prob(0, z, loc.expand(P, n), sc.expand(P, n)).sum()


def tail_reference(sites, inp, epss, P, coef_all, xcoef, clipped, dtype):
    """-> dict total, d_value [per site, [P, n]], grad (the flat gradient after the backward, before Adam),
    p, m, v after one optimizer step: float64 numpy.  ``epss``: the draw's eps per site, [P, n] numpy.  The prior
    entry has coefficient 1, the guide entry -1."""
    t = lambda x: torch.as_tensor(x, dtype=dtype)   # noqa: E731
    flat = t(inp["p"]).clone().requires_grad_(True)
    total = torch.zeros((), dtype=dtype)
    scalar = torch.zeros((), dtype=dtype)
    d_values = []
    for k_, (s, eps) in enumerate(zip(sites, epss)):
        n = s[0]
        lo, ro = inp["locs"][k_][0], inp["rhos"][k_][0]
        loc, rho = flat[lo:lo + n], flat[ro:ro + n]
        sc = torch.nn.functional.softplus(rho, threshold=20)
        z = loc + sc * t(eps)
        lp, lq = _tail_site_terms(s, loc, sc, z, P, t, dtype)
        total = total + (lp - lq)
        scalar = scalar + coef_all * (lp - lq)
        if xcoef is not None:
            scalar = scalar + coef_all * xcoef * (t(inp["extra"][k_]) * z).sum()
        # d_value: the gradient with respect to z alone, the guide's parameters held fixed
        zl = z.detach().clone().requires_grad_(True)
        lp, lq = _tail_site_terms(s, loc.detach(), sc.detach(), zl, P, t, dtype)
        sz = coef_all * (lp - lq)
        if xcoef is not None:
            sz = sz + coef_all * xcoef * (t(inp["extra"][k_]) * zl).sum()
        d_values.append(torch.autograd.grad(sz, zl)[0].double().numpy())
    grad, = torch.autograd.grad(scalar, flat)
    g_np = (grad + t(inp["g"])).double().numpy()
    hy = dict(TAIL_HYPER) if clipped else dict(TAIL_HYPER, clip=0.0, lrd=1.0)
    with np.errstate(all="ignore"):
        step = gc.torch_clipped_adam_step if clipped else gc.torch_adam_step
        p, m_, v = step(inp["p"], g_np, inp["m"], inp["v"], TAIL_STEP0, hy, dtype)
    return dict(total=float((coef_all * total).detach().double()), d_value=d_values, grad=g_np, p=p, m=m_, v=v, hy=hy)


def tail_magnitudes(sites, inp, epss, P, coef_all, xcoef, ref, clipped):
    """M of the total, of d_value per site, of the flat gradient, and of the Adam outputs.  The gradient is itself
    a sum: the optimizer's M is guide_edge_cases.adam_magnitudes with |g| replaced by the gradient's M (and no
    clamp: a clamp passes an error of its argument on unchanged or not at all)."""
    Mg = np.abs(inp["g"]).copy()
    Mtot, Mdv = 0.0, []
    w = abs(coef_all)
    bc = lambda x, n: np.broadcast_to(np.asarray(x, np.float64), (P, n))   # noqa: E731
    for k_, (s, eps) in enumerate(zip(sites, epss)):
        n, prior, p0, p1, m = s
        lo, ro = inp["locs"][k_][0], inp["rhos"][k_][0]
        loc, rho = inp["p"][lo:lo + n], inp["p"][ro:ro + n]
        sc = softplus(rho, F64)
        z = loc[None, :] + sc[None, :] * eps
        Mp = ec.magnitude(prior, z, bc(p0.numpy().reshape(1, 1), n), bc(p1.numpy().reshape(1, 1), n))
        Mq = ec.magnitude(0, z, bc(loc[None, :], n), bc(sc[None, :], n))
        Mp = {k2: np.broadcast_to(x, (P, n)) for k2, x in Mp.items()}
        if m is not None:
            Mp = {k2: np.where(m.reshape(P, n).numpy(), x, 0.0) for k2, x in Mp.items()}
        Mtot += w * float(np.sum(Mp["lp"]) + np.sum(Mq["lp"]))
        dz = w * (Mp["dv"] + Mq["dv"])
        if xcoef is not None:
            dz = dz + w * abs(xcoef) * np.abs(inp["extra"][k_])
        Mdv.append(dz)
        sig = 1.0 / (1.0 + np.exp(-rho))
        Mg[lo:lo + n] += dz.sum(0) + w * Mq["da"].sum(0)
        Mg[ro:ro + n] += sig * ((dz * np.abs(eps)).sum(0) + w * Mq["db"].sum(0))
    hy = dict(ref["hy"], clip=INF) if clipped else ref["hy"]
    Mp_, Mm_, Mv_ = gc.adam_magnitudes(inp["p"], Mg, inp["m"], inp["v"], TAIL_STEP0, hy, clipped, ref["v"])
    return dict(total=Mtot, d_value=Mdv, grad=Mg, p=Mp_, m=Mm_, v=Mv_)


def tail_k(sites, P):
    """Terms one thread adds, per flat-gradient element: the guide entry's reduced parameter gradient (ROWRED on
    [P, n]; COLRED on a scalar site's [1, P]) and the backward's sum over the particles, one after the other."""
    out = []
    for s in sites:
        n = s[0]
        kq = k_grad(1, P, 1, "colred") if n == 1 else k_grad(P, n, 1, "rowred")
        out.append(kq + k_bwd(n, P) + 2)
    return out
