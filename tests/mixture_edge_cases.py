"""Grids, input builders, float64 references, magnitudes and launch-plan restatements of the six mixture leaves
(csrc/mixture.hip, mixture_rows.hip, mixture_event.hip + .h, mixture_mvn.hip + .h): shared by
test_mixture_edges_host.py (CPU) and test_mixture_edges_gpu.py (the HIP kernels).

Reference: float64 torch on the CPU, independent of the kernels and of oracle/: the explicit frame

    t[b, n, k] = a[b, (n,) k] + sum_d log p(x[n, d] | p0[b, k, d], p1[b, k, d])     (dist_edge_cases.torch_log_prob)
    lse = torch.logsumexp(t, k),   S[b] = sum_n lse,   r = softmax_k t,
    R[b, k] = sum_n r,   dS/dp[b, k, d] = sum_n r dlogp/dp                            (autograd, per element)

and for the full-covariance leaf the statistics of mvn_mixture_cases.mvn_leaf_reference (S, R, m = sum r z,
G = tril sum r z d^T, z = W d, d = x - loc) on the same explicit [B, K, N, D] frame.  Two conventions, the project's
(enum_edge_cases.py, mixture_lanes.h):
  a dead row   (every term -inf) has lse = -inf -- S = -inf for that set -- and no responsibilities: it adds exactly
               nothing to R or to a parameter gradient, whatever the family's derivative is there;  likewise a
               responsibility that is exactly 0 (a switched-off or collapsed component) adds exactly nothing;
  a NaN term   follows torch: the row's lse and every r of the row are NaN, hence S, every R_k and every
               parameter-gradient entry of that set.
torch.distributions.LogNormal at x = 0 is -inf - log 0 = NaN: under this reference such a row is a NaN row, not a
dead one (the scalar kernels compute the same difference); Gamma(alpha > 1) at x = 0 and a Normal at x = inf are dead.

Tolerance: the rule of dist_edge_cases.check, per output ENTRY:
  float64  the non-finite pattern equals the reference's exactly; elsewhere |got - ref64| <= 64 eps64 M.
  float32  |got - ref64| <= 4 |cpu32 - ref64| + (8 + k / 2) eps32 M, cpu32 = the same torch formula in float32 on
           the CPU, k = the largest number of working-type additions one thread makes before the partial sums go to
           double (the amendment of multisite_edge_cases.py), from the thread maps restated below:
             scalar / diag / rows / rows-diag   rows per lane = ceil(N / (grid * 4 * (64 / KP)))       (lane_plan)
             event   DC features per chunk for t (S), TB = DC rows per sub-tile for the statistics     (event_plan)
             MVN     TR rows per tile for C, s and R (256; 128 for float64 at DP = 64)                 (mvn_plan)
  M        term magnitudes from dist_edge_cases.magnitude plus |a_k|, weighted by the float64 responsibilities and
           summed over d and over the rows that enter the entry, as test_dist_edges_gpu.py builds them for the scalar
           leaf; for the MVN leaf the |W| (|x| + |loc|) magnitudes of the products behind m and G.
Every input is representable in float32, so one float64 reference serves both dtypes; every device input is a
contiguous view inside a larger NaN-filled buffer (layer_edge_cases.embed): a read past N or past D that is USED
shows up as a NaN.

Unscored elements (cpu32 non-finite where ref64 is finite): 0 on the geometry grids, at most 5 % of an edge case
(test_mixture_edges_host.py asserts both from the references alone).  The edge grids take their points from
dist_edge_cases.grid(f32=True) minus the points whose float32 torch result is non-finite while float64 is finite and
minus infinite operands (those are the subject of the non-finite cases).

Exact cases need no tolerance: components 1e4 apart with unit scales (W = I), integer data at integer offsets of
magnitude <= 8 from integer locs.  Every responsibility is exactly 0 or 1 in both dtypes and every partial sum an
integer below 2^24, so R, dloc = sum (x - loc), dscale = sum ((x - loc)^2 - 1), m and the lower triangle of G must
torch.equal the integer counts and sums.  The row pattern leaves components with 0, 1 and 2 rows.

Defects the suite found (all by the non-finite cases; the kernels are fixed, the assertions stay):
  1. mixture.hip, both kernels: mix_max(a, b) = a > b ? a : b returned b for a NaN a and NaN for a NaN b, so the lanes
     of a butterfly step disagreed and a NaN term gave S = -inf or S = NaN depending on the component that held it.
     Fixed: mix_nanmax / mix_row in mixture_lanes.h (the row helper mixture_rows.hip had), used by all four kernels.
  2. mixture_kernel: `r > 0 ? r * da : 0` dropped a NaN r: S and R NaN, parameter gradients finite.  Fixed:
     `r == 0 ? 0 : r * da`.
  3. 0 * inf from rows or components with r = 0: mixture_diag_kernel (w * z, w * (z z - 1): a dead row, and in float32
     a live row with a collapsed component whose z z overflows), mixture_event_stats_kernel (r * statistic: Gamma at
     x = 0, Normal at x = inf), mixture_mvn_stats_kernel (r * d in C and s).  Fixed: an exactly-zero r adds nothing
     (diag: a branch around the sums; event: a second launch of the stats kernel that adds a record again, without
     the zero responsibilities, where the plain launch left it non-finite; MVN: d staged as 0 for such a row).
  4. mixture_diag_kernel: the padded features d >= D computed (x[row][0] - mu) * 0: NaN for x[row][0] = inf, a NaN row
     instead of a dead one.  Fixed: a padded slot reads mu itself as its value, so x - mu = 0 there.
  5. mixture_event_lse_kernel: a row term of +inf beside a logsumexp of -inf (LogNormal at x = 0) made S NaN while
     the statistics treated the row as dead (finite R and gradients).  Fixed: such a row's stored logsumexp is NaN, so
     R and the gradients are NaN with S, as the reference has them.
  6. mixture_event_finalize_kernel: the chain rule on the totals formed 0 / 0 for a component no row has a
     responsibility for when a factor is singular there (Poisson at rate 0: s / lam - R; found by the Poisson edge
     grid).  Fixed: R == 0 exactly gives a zero gradient.
The fixes change no finite result: PARENT_BITS holds one geometry case per fixed kernel as the parent commit computed
it, and test_fixed_kernels_keep_the_parents_bits compares bit for bit, in both dtypes.  That shaped the fixes: a select
or a branch inside the float32 sums changes how the compiler packs and fuses their multiply-adds, and with that the
last bits of ordinary data.  So the diag kernel spells out the three fused multiply-adds it always had in float32, and
the event leaf's guard lives in a launch of its own, which leaves the plain sums' code untouched.

Measured on the MI355X (256 CUs), largest error / bound per kernel and dtype over every case of the GPU suite
(test_zz_measured_constants prints them; every ratio must stay below 1):

    kernel       dtype   geometry   families   edge    non-finite   empty chunk
    scalar       f32     0.081      0.015      0.250   0.013
    scalar       f64     0.013      0.005      0.010   0.007
    rows         f32     0.154      0.121      0.148   0.105
    rows         f64     0.022      0.017      0.006   0.020
    diag         f32     0.122                 0.029   0.028
    diag         f64     0.019                 0.013   0.012
    rows_diag    f32     0.148                 0.060   0.154
    rows_diag    f64     0.022                 0.009   0.023
    event        f32     0.023      0.005      0.750   0.015        0.003
    event        f64     0.017      0.005      0.013   0.010        0.007
    mvn          f32     0.000                         0.000        0.001
    mvn          f64     0.003                         0.003        0.005
"""
import functools
import math

import numpy as np
import torch

from tests import dist_edge_cases as ec
from tests.dist_edge_cases import EPS32, EPS64, F32_TINY, check
from tests.layer_edge_cases import embed

F32, F64 = torch.float32, torch.float64
INF, NAN = math.inf, math.nan
NORMAL, BERNOULLI, LOG_NORMAL, EXPONENTIAL, GAMMA, POISSON = 0, 1, 3, 4, 6, 8
FAMILIES = (NORMAL, LOG_NORMAL, EXPONENTIAL, BERNOULLI, POISSON, GAMMA)
TWO_PARAM = (NORMAL, LOG_NORMAL, GAMMA)
MI355X_CUS = 256
UNSCORED_CAP = 0.05


def r32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def cdiv(a, b):
    return -(-a // b)


def dname(dtype):
    return "f32" if dtype == F32 else "f64"


# =====================================================================================================================
# cases
# =====================================================================================================================
class Case:
    """One leaf call: numpy float64 arrays representable in float32.  x [N, D]; a [B, K] or [B, N, K];
    p0, p1 [B | 1, K | 1, D | 1] (p1 None for a one-parameter family).  The references are computed once."""

    def __init__(self, dist_id, x, a, p0, p1, name=""):
        self.dist_id, self.name = dist_id, name
        self.x, self.a, self.p0 = r32(x), r32(a), r32(p0)
        self.p1 = None if p1 is None else r32(p1)
        self.N, self.D = self.x.shape
        self.B, self.K = self.a.shape[0], self.a.shape[-1]
        self.rows = self.a.ndim == 3
        self._ref = {}

    def ref(self, dtype=F64):
        if dtype not in self._ref:
            self._ref[dtype] = leaf_reference(self.dist_id, self.x, self.a, self.p0, self.p1, dtype)
        return self._ref[dtype]

    def mag(self):
        if "M" not in self._ref:
            self._ref["M"] = leaf_magnitudes(self.dist_id, self.x, self.a, self.p0, self.p1, self.ref(F64))
        return self._ref["M"]

    def modified(self, name="", **kw):
        """A copy with some arrays replaced (x=..., a=..., p0=..., p1=...)."""
        f = dict(x=self.x, a=self.a, p0=self.p0, p1=self.p1)
        f.update(kw)
        return Case(self.dist_id, f["x"], f["a"], f["p0"], f["p1"], name or self.name)


def _values(dist_id, g, shape):
    if dist_id == NORMAL:
        return g.standard_normal(shape)
    if dist_id == BERNOULLI:
        return (g.uniform(size=shape) < 0.5).astype(np.float64)
    if dist_id == POISSON:
        return g.integers(0, 6, shape).astype(np.float64)
    return g.uniform(0.1, 3.0, shape)


def _params(dist_id, g, shape):
    p0 = g.standard_normal(shape) if dist_id in (NORMAL, LOG_NORMAL, BERNOULLI) else g.uniform(0.5, 2.0, shape)
    p1 = g.uniform(0.5, 2.0, shape) if dist_id in TWO_PARAM else None
    return p0, p1


def _pshape(share, B, K, D):
    return (1 if "b" in share else B, 1 if "k" in share else K, 1 if "d" in share else D)


@functools.lru_cache(maxsize=None)
def geometry(dist_id, N, K, D, B, rows=False, share0="", share1="", share_a=False, seed=0):
    """Ordinary data: values randn, scales and rates in [0.5, 2], positive-support values in [0.1, 3], counts small
    integers, normalised log-weights.  share0 / share1: the axes ("k", "d", "b") over which p0 / p1 are shared;
    share_a: one set of weights for every b (rows leaves)."""
    g = np.random.default_rng(1000003 * seed + 7919 * dist_id + 31 * N + 17 * K + 5 * D + B)
    x = _values(dist_id, g, (N, D))
    w = g.standard_normal((1 if share_a else B, N, K) if rows else (B, K))
    a = w - np.log(np.exp(w).sum(-1, keepdims=True))
    if rows and share_a:
        a = np.broadcast_to(a, (B, N, K))
    p0, _ = _params(dist_id, g, _pshape(share0, B, K, D))
    _, p1 = _params(dist_id, g, _pshape(share1, B, K, D))
    return Case(dist_id, x, a, p0, p1, "geometry")


# ---- edge grids ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_points(dist_id):
    """(v, a, b) of dist_edge_cases.grid(f32=True) without infinite or NaN operands and without the points whose
    float32 torch result (value or parameter derivative) is non-finite while float64 is finite."""
    v, a, b = ec.grid(dist_id, True)
    keep = np.isfinite(v) & np.isfinite(a) & np.isfinite(b)
    v, a, b = v[keep], a[keep], b[keep]
    with np.errstate(all="ignore"):
        r64, r3 = ec.reference(dist_id, v, a, b, F64), ec.reference(dist_id, v, a, b, F32)
    names = ("lp", "da", "db") if dist_id in TWO_PARAM else ("lp", "da")
    ok = np.ones(v.shape, bool)
    for q in names:
        ok &= ~(np.isfinite(r64[q]) & ~np.isfinite(r3[q]))
    ok &= np.isfinite(r64["lp"])
    return v[ok], a[ok], b[ok]


@functools.lru_cache(maxsize=None)
def edge_case(dist_id, K, D, rows=False, seed=0):
    """A mixture over the family's edge points: component (k, d) takes the parameters of one grid point, the rows take
    the values of the grid points; the rows that float32 cannot score are thinned out (see below), which keeps every
    output within the 5 % cap of the rule."""
    v, a, b = edge_points(dist_id)
    g = np.random.default_rng(97 * dist_id + 13 * K + D + seed)
    par = sorted({(pa, pb) for pa, pb in zip(a, b)})
    idx = g.permutation(len(par))[:K * D]
    idx = np.resize(idx, K * D)
    p0 = np.array([par[i][0] for i in idx]).reshape(1, K, D)
    p1 = np.array([par[i][1] for i in idx]).reshape(1, K, D) if dist_id in TWO_PARAM else None
    vals = np.unique(v)
    x = vals[g.integers(0, vals.size, (6 * vals.size, D))]
    N = x.shape[0]
    w = np.log(np.arange(1, K + 1) / (K * (K + 1) / 2))
    a_ = np.broadcast_to(w, (1, N, K)).copy() if rows else w[None, :]
    if rows:
        a_ = a_ + 0.25 * g.standard_normal(a_.shape)
    # keep the rows that are live and whose every contribution (lse, r dlogp/dp per (k, d)) is finite in float64 and
    # in float32: dead and NaN rows are the subject of the non-finite cases, and a row that float32 cannot score
    # would take the whole sum with it
    cand = Case(dist_id, x, a_, p0, p1)
    keep = np.ones(N, bool)
    with np.errstate(all="ignore"):
        for dt in (F64, F32):
            ref = cand.ref(dt)
            rr = ref["r"][0][..., None]
            keep &= np.isfinite(ref["lse"][0])
            for q in ("ge0", "ge1"):
                keep &= np.isfinite(np.where(rr == 0, 0.0, rr * ref[q][0])).all((1, 2))
    x, a_ = x[keep], (a_[:, keep] if rows else a_)
    return Case(dist_id, x, a_, p0, p1, "edge")


# ---- the exact cases -------------------------------------------------------------------------------------------------
def exact_rows(N, K):
    """The component of every row: component 1 owns no row, 2 one row, 3 two rows (where they exist), the others
    take turns."""
    rest = [k for k in range(K) if k not in (1, 2, 3)] or [0]
    z = np.array([rest[n % len(rest)] for n in range(N)])
    if K > 2 and N > 0:
        z[0] = 2
    if K > 3 and N > 2:
        z[1] = z[2] = 3
    return z


def exact_case(N, K, D, B=1, rows=False):
    """(Case, expected): integer data around components 1e4 apart; expected = dict R [K], dloc [K, D], dscale [K, D],
    G [K, D, D] (lower triangle of sum off off^T) and z [N], all integers in float64."""
    z = exact_rows(N, K)
    loc = 1e4 * np.arange(K)[:, None] + np.arange(D)[None, :]
    off = ((np.arange(N)[:, None] * 7 + np.arange(D)[None, :] * 3) % 17 - 8).astype(np.float64)
    x = loc[z] + off
    a = np.zeros((B, N, K) if rows else (B, K))
    case = Case(NORMAL, x, a, loc[None], np.ones((1, K, D)), "exact")
    onehot = (z[:, None] == np.arange(K)[None, :]).astype(np.float64)            # [N, K]
    exp = dict(z=z, R=onehot.sum(0), dloc=onehot.T @ off, dscale=onehot.T @ (off * off - 1.0),
               G=np.tril(np.einsum("nk,ni,nj->kij", onehot, off, off)), r=onehot)
    assert np.abs(exp["dscale"]).max() < 2 ** 24 and np.abs(x).max() < 2 ** 24
    return case, exp


# =====================================================================================================================
# the references
# =====================================================================================================================
def leaf_reference(dist_id, x, a, p0, p1, dtype=F64):
    """dict of numpy float64: S [B], R [B, K], r [B, N, K], lse [B, N], g0, g1 [B, K, D] (per (b, k, d): a shared
    parameter's gradient is NOT summed, as the kernels return it), and the per-element ge0, ge1, lp [B, N, K, D] --
    torch evaluated in ``dtype`` on the explicit frame."""
    N, D = x.shape
    B, K = a.shape[0], a.shape[-1]
    full = (B, N, K, D)
    two = p1 is not None
    tx = torch.tensor(x, dtype=dtype)[None, :, None, :].expand(full)
    P0 = torch.tensor(p0, dtype=dtype)[:, None].expand(full).clone().requires_grad_(True)
    P1 = (torch.tensor(p1, dtype=dtype)[:, None].expand(full).clone().requires_grad_(True) if two
          else torch.zeros(full, dtype=dtype))
    lp = ec.torch_log_prob(dist_id, tx, P0, P1)
    gs = torch.autograd.grad(lp.sum(), [P0, P1] if two else [P0])
    ge0, ge1 = gs[0], (gs[1] if two else torch.zeros(full, dtype=dtype))
    lp = lp.detach()
    ta = torch.tensor(a, dtype=dtype)
    t = (ta if ta.dim() == 3 else ta[:, None, :]) + lp.sum(-1)                    # [B, N, K]
    lse = torch.logsumexp(t, -1)
    dead = lse == -INF
    r = torch.where(dead[..., None], torch.zeros_like(t), torch.softmax(t, -1))
    rr = r[..., None]
    zero = torch.zeros(full, dtype=dtype)
    out = dict(S=lse.sum(1), R=r.sum(1), r=r, lse=lse, g0=torch.where(rr == 0, zero, rr * ge0).sum(1),
               g1=torch.where(rr == 0, zero, rr * ge1).sum(1), ge0=ge0, ge1=ge1, lp=lp)
    return {k: v.double().numpy() for k, v in out.items()}


def leaf_magnitudes(dist_id, x, a, p0, p1, ref):
    """M per output entry (dict S, R, r, g0, g1), from the float64 reference ``ref``."""
    N, D = x.shape
    B, K = a.shape[0], a.shape[-1]
    full = (B, N, K, D)
    with np.errstate(all="ignore"):
        Mt = ec.magnitude(dist_id, np.broadcast_to(x[None, :, None, :], full), np.broadcast_to(p0[:, None], full),
                          np.broadcast_to(p1[:, None] if p1 is not None else 0.0, full))
        aa = np.abs(a if a.ndim == 3 else a[:, None, :])
        Mterm = aa + np.broadcast_to(Mt["lp"], full).sum(-1)                     # [B, N, K]
        r = ref["r"]
        pos = r > 0
        Mrow = np.where(pos, r * Mterm, 0.0).sum(-1) + 1.0                       # [B, N]
        Mr = np.where(pos, Mterm + Mrow[..., None], 0.0)                         # a responsibility's error, relative
        live = np.isfinite(ref["lse"])
        M = dict(S=np.where(live, Mrow, 0.0).sum(1), r=np.where(pos, r * (1.0 + Mr), 0.0))
        M["R"] = M["r"].sum(1)
        for q, name, ge in (("da", "g0", ref["ge0"]), ("db", "g1", ref["ge1"])):
            Mq = np.broadcast_to(np.abs(Mt[q]), full)
            M[name] = np.where(pos[..., None], r[..., None] * (Mq + np.abs(ge) * Mr[..., None]), 0.0).sum(1)
    return M


class MvnCase:
    """x [N, D]; a [B, K]; loc [B | 1, K | 1, D]; W [B | 1, K | 1, D, D] lower triangular (representable in float32)."""

    def __init__(self, x, a, loc, W, name=""):
        self.x, self.a, self.loc, self.W, self.name = r32(x), r32(a), r32(loc), np.tril(r32(W)), name
        self.N, self.D = self.x.shape
        self.B, self.K = self.a.shape
        self._ref = {}

    def ref(self, dtype=F64):
        if dtype not in self._ref:
            self._ref[dtype] = mvn_reference(self.x, self.a, self.loc, self.W, dtype)
        return self._ref[dtype]

    def mag(self):
        if "M" not in self._ref:
            self._ref["M"] = mvn_magnitudes(self.x, self.a, self.loc, self.W, self.ref(F64))
        return self._ref["M"]

    def modified(self, name="", **kw):
        f = dict(x=self.x, a=self.a, loc=self.loc, W=self.W)
        f.update(kw)
        return MvnCase(f["x"], f["a"], f["loc"], f["W"], name or self.name)


@functools.lru_cache(maxsize=None)
def mvn_geometry(N, K, D, B, share_loc="", share_w="", seed=0, dense=False):
    """Ordinary data: x around K centres, W = the inverse of a well-conditioned lower-triangular scale factor
    (``dense``: every entry below the diagonal away from zero)."""
    g = np.random.default_rng(424243 * seed + 8191 * N + 131 * K + 7 * D + B)
    centres = 2.0 * g.standard_normal((K, D))
    x = centres[g.integers(0, K, N)] + g.standard_normal((N, D))
    w = g.standard_normal((B, K))
    a = w - np.log(np.exp(w).sum(-1, keepdims=True))
    ls = (1 if "b" in share_loc else B, 1 if "k" in share_loc else K, D)
    loc = centres[None, :ls[1]] + 0.3 * g.standard_normal(ls)
    ws = (1 if "b" in share_w else B, 1 if "k" in share_w else K, D, D)
    low = g.standard_normal(ws) * 0.3 / math.sqrt(D)
    if dense:
        low = np.sign(low) * (np.abs(low) + 0.05)
    W = np.tril(low, -1) + np.eye(D) * g.uniform(0.5, 2.0, ws[:3])[..., None]
    return MvnCase(x, a, loc, W, "geometry")


def mvn_reference(x, a, loc, W, dtype=F64):
    """dict of numpy float64: S [B], R [B, K], m [B, K, D], G [B, K, D, D] (zero above the diagonal), lse [B, N],
    r [B, K, N] and the frame's z, d [B, K, N, D] -- torch in ``dtype``."""
    N, D = x.shape
    B, K = a.shape
    tx, ta = torch.tensor(x, dtype=dtype), torch.tensor(a, dtype=dtype)
    tl = torch.tensor(loc, dtype=dtype).expand(B, K, D)
    tW = torch.tril(torch.tensor(W, dtype=dtype)).expand(B, K, D, D)
    d = tx[None, None] - tl[:, :, None, :]                                        # [B, K, N, D]
    # (z_i = sum_{j <= i} W_ij d_j: the structural zeros above the diagonal are no factors -- 0 * inf is not formed)
    low = torch.tril(torch.ones(D, D, dtype=torch.bool))
    prod = tW[:, :, None, :, :] * d[:, :, :, None, :]                             # [B, K, N, D, D]
    z = torch.where(low, prod, torch.zeros_like(prod)).sum(-1)
    logdet = torch.log(torch.diagonal(tW, dim1=-2, dim2=-1)).sum(-1)
    t = (ta + logdet)[:, :, None] - 0.5 * D * math.log(2 * math.pi) - 0.5 * (z * z).sum(-1)
    lse = torch.logsumexp(t, 1)                                                   # [B, N]
    dead = lse == -INF
    r = torch.where(dead[:, None, :], torch.zeros_like(t), torch.softmax(t, 1))   # [B, K, N]
    none = (r == 0)[..., None]
    rz = torch.where(none, torch.zeros_like(z), r[..., None] * z)
    dz = torch.where(none, torch.zeros_like(d), d)
    out = dict(S=lse.sum(-1), R=r.sum(-1), m=rz.sum(2), G=torch.tril(torch.einsum("bkni,bknj->bkij", rz, dz)),
               lse=lse, r=r, z=z, d=d)
    return {k: v.double().numpy() for k, v in out.items()}


def mvn_magnitudes(x, a, loc, W, ref):
    N, D = x.shape
    B, K = a.shape
    with np.errstate(all="ignore"):
        Wf = np.broadcast_to(np.abs(W), (B, K, D, D))
        Ad = np.abs(x)[None, None] + np.broadcast_to(np.abs(loc), (B, K, D))[:, :, None, :]      # [B, K, N, D]
        Mz = np.einsum("bkij,bknj->bkni", Wf, Ad)
        ld = np.abs(np.log(np.diagonal(Wf, axis1=-2, axis2=-1))).sum(-1)
        Mterm = (np.abs(a) + ld)[:, :, None] + 0.5 * D * math.log(2 * math.pi) + 0.5 * (Mz * Mz).sum(-1)   # [B, K, N]
        r = ref["r"]
        pos = r > 0
        Mrow = np.where(pos, r * Mterm, 0.0).sum(1) + 1.0                                        # [B, N]
        Mr = np.where(pos, Mterm + Mrow[:, None, :], 0.0)
        live = np.isfinite(ref["lse"])
        Mresp = np.where(pos, r * (1.0 + Mr), 0.0)
        rp = np.where(pos, r, 0.0)
        az, ad = np.where(pos[..., None], np.abs(ref["z"]), 0.0), np.where(pos[..., None], np.abs(ref["d"]), 0.0)
        Mzp, Adp = np.where(pos[..., None], Mz, 0.0), np.where(pos[..., None], Ad, 0.0)
        M = dict(S=np.where(live, Mrow, 0.0).sum(1), R=Mresp.sum(-1),
                 m=(rp[..., None] * (Mzp + az * Mr[..., None])).sum(2),
                 G=np.einsum("bkn,bkni,bknj->bkij", rp, Mzp, Adp) +
                 np.einsum("bkn,bkni,bknj->bkij", rp * Mr, az, ad))
    return M


# =====================================================================================================================
# the rule
# =====================================================================================================================
RATIOS = {}          # label -> the largest error / bound seen


def unscored(ref64, cpu32):
    ref64, cpu32 = np.asarray(ref64, np.float64), np.asarray(cpu32, np.float64)
    return int((np.isfinite(ref64) & ~np.isfinite(cpu32)).sum())


def score(label, what, got, ref64, M, f32, cpu32=None, k=0):
    """dist_edge_cases.check per entry with the reduced-output amendment: in float32 the last term of the bound is
    (8 + k / 2) eps32 M (k = 0: an un-reduced output).  In float32 the non-finite pattern is compared too wherever
    cpu32 has the reference's.  Records error / bound under ``label``."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, "%s %s: shape %s, reference %s" % (label, what, got.shape, ref64.shape)
    M = np.broadcast_to(np.asarray(M, np.float64), got.shape)
    Meff = M * ((8 + k / 2) / 8) if f32 else M
    with np.errstate(all="ignore"):
        if f32:
            cpu32 = np.broadcast_to(np.asarray(cpu32, np.float64), got.shape)
            bound = 4 * np.abs(cpu32 - ref64) + 8 * EPS32 * Meff + F32_TINY
            scored = np.isfinite(cpu32) & np.isfinite(ref64) & np.isfinite(got)
            nf = ~np.isfinite(ref64) & ((cpu32 == ref64) | (np.isnan(cpu32) & np.isnan(ref64)))
            bad = nf & ~((got == ref64) | (np.isnan(got) & np.isnan(ref64)))
            assert not bad.any(), "%s %s: non-finite pattern differs at %s: got %s, reference %s" % (
                label, what, np.argwhere(bad)[:4].tolist(), got[bad][:4], ref64[bad][:4])
        else:
            bound = 64 * EPS64 * Meff
            scored = np.isfinite(ref64) & np.isfinite(got)
        err = np.where(got == ref64, 0.0, np.abs(got - ref64))
        ratio = np.where(scored, err / np.where(bound > 0, bound, 1.0), 0.0)
        ratio = np.where(scored & (bound == 0) & (err > 0), np.inf, ratio)
    if ratio.size:
        RATIOS[label] = max(RATIOS.get(label, 0.0), float(ratio.max()))
    check("%s %s" % (label, what), got, ref64, Meff, f32, cpu32)


def score_leaf(label, case, out, dtype, ks, want=("S", "R", "g0", "g1", "r")):
    """Every output of a lane-layout or event leaf (dict S [B], R [B, K], g0, g1 [B, K, D], r [B, N, K] or None)
    against the case's references.  ks: dict output -> k of the amendment."""
    f32 = dtype == F32
    ref, M = case.ref(F64), case.mag()
    c32 = case.ref(F32) if f32 else None
    for q in want:
        if out.get(q) is None or (q == "g1" and case.p1 is None):
            continue
        score(label, "%s %s %s" % (case.name, q, dname(dtype)), out[q], ref[q], M[q], f32,
              None if c32 is None else c32[q], ks.get(q, 0))


def score_mvn(label, case, out, dtype, k):
    f32 = dtype == F32
    ref, M = case.ref(F64), case.mag()
    c32 = case.ref(F32) if f32 else None
    for q in ("S", "R", "m", "G"):
        score(label, "%s %s %s" % (case.name, q, dname(dtype)), out[q], ref[q], M[q], f32,
              None if c32 is None else c32[q], k)
    up = np.triu(np.ones((case.D, case.D), bool), 1)
    assert (out["G"][..., up] == 0).all(), "%s: G is not exactly zero above the diagonal" % label


# =====================================================================================================================
# the launch plans, restated
# =====================================================================================================================
MIX_THREADS, MIX_WAVES, MIX_U = 256, 4, 4
EV_TR, EV_KC, EV_THREADS = 256, 16, 256
EV_LSE_BLOCKS, EV_STAT_BLOCKS, EV_REC_CAP = 2048, 1024, 40.0 * 1024 * 1024
MVN_THREADS, MVN_LSE_BLOCKS, MVN_STAT_BLOCKS = 256, 2048, 1024


def kp_of(K):
    kp = 1
    while kp < K:
        kp <<= 1
    return kp


def dd_of(D):
    return 2 if D <= 2 else 4 if D <= 4 else 8


def rb_of(K):
    """Rows per workgroup iteration of the lane-layout kernels."""
    return MIX_WAVES * (64 // kp_of(K))


def lane_plan(N, K, B, cus, per_cu):
    """mixture_grid / mixr_grid (per_cu = 4) and mixture_diag_blocks / the diag mixr_grid (per_cu = 2): dict grid,
    KP, rows_per_lane (= k of the rule) and nparts (partials of the second launch: workgroups, or waves for the
    diag kernels -- the caller multiplies)."""
    KP = kp_of(K)
    rows_per_block = MIX_WAVES * (64 // KP)
    g = cdiv(N, rows_per_block * 8)
    cap = max(1, cdiv(cus * per_cu, B))
    grid = max(1, min(g, cap))
    return dict(grid=grid, KP=KP, rows_per_lane=cdiv(N, grid * rows_per_block))


def lane_walk(N, K, grid, unroll=MIX_U):
    """A brute-force walk of the kernels' row loop (``unroll`` iterations whose loads are requested together, with the
    wave-uniform break): {(workgroup, wave, slot): [rows]}.  unroll = 1: mixture_diag_kernel's plain loop."""
    KP = kp_of(K)
    rpw = 64 // KP
    step = grid * MIX_WAVES * rpw
    owner = {}
    for wg in range(grid):
        for wave in range(MIX_WAVES):
            base0 = (wg * MIX_WAVES + wave) * rpw
            while base0 < N:
                for u in range(unroll):
                    base = base0 + u * step
                    if base >= N:
                        break
                    for slot in range(rpw):
                        if base + slot < N:
                            owner.setdefault((wg, wave, slot), []).append(base + slot)
                base0 += unroll * step
    return owner


def partial_segments(nparts):
    """The second launch: 16 segments of ceil(nparts / 16) partials, each an 8-deep loop and a remainder:
    [(b0, b1, eights, rest)]."""
    per = cdiv(nparts, 16)
    segs = []
    for sg in range(16):
        b0 = sg * per
        b1 = min(b0 + per, nparts)
        n = max(0, b1 - b0)
        segs.append((b0, b1, n // 8, n % 8))
    return segs


def ev_nx(dist_id):
    return 2 if dist_id == GAMMA else 1


def ev_ns(dist_id):
    return 2 if dist_id in TWO_PARAM else 1


def event_plan(dist_id, K, D, B, N, f32):
    """mixture_event_launch: dict DB, nkc, ndb, DC (= TB), g1, chunks, rows_per, chunk_rows [(r0, r1)]."""
    DB = 16 if D <= 16 else 64 if D <= 64 else 256
    NS = ev_ns(dist_id)
    nkc, ndb = cdiv(K, EV_KC), cdiv(D, DB)
    groups = B * nkc * ndb
    record = EV_KC + EV_KC * DB * NS
    cmax = cdiv(EV_STAT_BLOCKS, groups)
    cmax = max(1, min(cmax, int(EV_REC_CAP / (8.0 * groups * record))))
    tiles = cdiv(N, EV_TR)
    chunks = min(tiles, cmax)
    rows_per = cdiv(cdiv(N, chunks), EV_TR) * EV_TR
    g1 = min(tiles, max(1, cdiv(EV_LSE_BLOCKS, B)))
    DC = (16 if f32 else 8) // ev_nx(dist_id)
    return dict(DB=DB, NS=NS, nkc=nkc, ndb=ndb, DC=DC, TB=DC, g1=g1, chunks=chunks, rows_per=rows_per,
                record=record, chunk_rows=[(c * rows_per, min(c * rows_per + rows_per, N)) for c in range(chunks)])


def event_pairs(DB):
    """mixture_event_stats_kernel: {(k, dl): [threads]} -- thread tid owns the pairs (tid // DB + j (256 / DB),
    tid % DB), j < 16 DB / 256."""
    ppt, kstep = EV_KC * DB // EV_THREADS, EV_THREADS // DB
    own = {}
    for tid in range(EV_THREADS):
        for j in range(ppt):
            own.setdefault((tid // DB + j * kstep, tid % DB), []).append(tid)
    return own


def mvn_plan(K, D, B, N, f32):
    """mixture_mvn_launch: dict DP, TB, NB, TR, g1, chunks, rows_per, chunk_rows."""
    DP = 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64
    TR = 128 if (not f32 and DP == 64) else 256
    cmax = max(1, cdiv(MVN_STAT_BLOCKS, K * B))
    tiles = cdiv(N, TR)
    chunks = min(tiles, cmax)
    rows_per = cdiv(cdiv(N, chunks), TR) * TR
    TB = DP // 16 if DP >= 16 else 1
    return dict(DP=DP, TB=TB, NB=DP // TB, TR=TR, g1=min(cdiv(N, MVN_THREADS), max(1, cdiv(MVN_LSE_BLOCKS, B))),
                chunks=chunks, rows_per=rows_per,
                chunk_rows=[(c * rows_per, min(c * rows_per + rows_per, N)) for c in range(chunks)])


def mvn_blocks(DP):
    """mixture_mvn_stats_kernel: {(bi, bj): [threads]} of the blocks of C on or below the diagonal, from the
    kernel's `while (bj > bi) bj -= ++bi` walk of tid < NLOW."""
    TB = DP // 16 if DP >= 16 else 1
    NB = DP // TB
    own = {}
    for tid in range(NB * (NB + 1) // 2):
        bi, bj = 0, tid
        while bj > bi and bi < NB:
            bi += 1
            bj -= bi
        own.setdefault((bi, bj), []).append(tid)
    return own


# =====================================================================================================================
# the grids of the GPU suite (host-checkable: the host test walks the same lists)
# =====================================================================================================================
LANE_K = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
DIAG_D = (1, 2, 3, 4, 5, 7, 8)
ROW_LAYOUTS = ("rows", "cols", "sliced", "shared")


def lane_ns(K):
    rb = rb_of(K)
    return sorted({1, max(1, rb - 1), rb, rb + 1, 4 * rb + 1, 8 * rb + 1, 33 * rb + 3})


LANE_DEEP = {"scalar": (64, 4231), "rows": (64, 4231), "diag": (64, 1100), "rows_diag": (64, 1100)}

# (K, D, N, B, share0, share1): every K, D, N, B and sharing of the list at the smallest partners
EVENT_SEAMS = (
    (1, 1, 1, 1, "", ""), (15, 7, 255, 1, "", ""), (16, 8, 256, 3, "", "k"), (17, 9, 257, 1, "k", ""),
    (33, 15, 513, 1, "", "d"), (64, 16, 257, 1, "d", ""), (17, 17, 257, 3, "b", "b"), (2, 64, 255, 1, "", ""),
    (3, 65, 257, 1, "", ""), (2, 256, 257, 1, "", "kd"), (2, 257, 256, 1, "", ""), (17, 65, 513, 1, "", ""),
    (33, 257, 1, 1, "", ""),
)
EVENT_WIDE = (2, 1024, 257, 1, "", "")
# an empty trailing chunk of the stats launch (test_mixture_edges_host.py derives it from event_plan)
EVENT_EMPTY_CHUNK = (49, 1, 1025, 64)       # K, D, N, B

# (D, K, N, B, share_loc, share_w)
MVN_SEAMS = (
    (1, 1, 1, 1, "", ""), (7, 3, 127, 1, "", ""), (8, 17, 128, 3, "", "k"), (9, 3, 129, 1, "k", ""),
    (16, 64, 255, 1, "", ""), (17, 3, 256, 3, "b", "b"), (32, 3, 257, 1, "", ""), (33, 3, 513, 1, "", "k"),
    (63, 1, 129, 1, "", ""), (64, 3, 257, 1, "", ""), (64, 1, 127, 3, "", "b"),
)
MVN_EMPTY_CHUNK = (64, 2, 1280, 4)          # K, D, N, B

# (K, D, per-row weights) of the edge cases: D = 1 feeds the scalar and rows leaves too, D = 2 the diag and event ones
EDGE_SHAPES = ((3, 1, False), (5, 1, True), (3, 2, False), (5, 2, True))


# =====================================================================================================================
# the device side: one call of a leaf on a case (test_mixture_edges_gpu.py)
# =====================================================================================================================
KINDS = ("scalar", "rows", "diag", "rows_diag", "event", "mvn")


def to_dev(arr, dtype, dev):
    """The array as a contiguous view inside a larger NaN-filled device buffer."""
    return embed(torch.tensor(np.ascontiguousarray(arr), dtype=dtype, device=dev))


def _flat(p, dtype, dev):
    """p [B0, K0, 1] -> (flat tensor, component stride, set stride) of the scalar leaves."""
    if p is None:
        return None, 0, 0
    B0, K0, _ = p.shape
    return to_dev(p.reshape(-1), dtype, dev), (1 if K0 > 1 else 0), (K0 if B0 > 1 else 0)


def _row_weights(a, layout, dtype, dev):
    """a [B, N, K] on the device in one of the layouts of ROW_LAYOUTS (a view of shape [B, N, K])."""
    B, N, K = a.shape
    if layout == "rows":
        return to_dev(a, dtype, dev)
    if layout == "cols":                # [K, N]-contiguous memory seen as [N, K]
        return to_dev(a.transpose(0, 2, 1), dtype, dev).transpose(1, 2)
    if layout == "sliced":              # the first K of K + 3 columns of a wider row-major matrix (NaN beside them)
        wide = np.full((B, N, K + 3), NAN)
        wide[..., :K] = a
        return to_dev(wide, dtype, dev)[..., :K]
    assert layout == "shared" and all((a[b] == a[0]).all() or np.isnan(a).any() for b in range(B))
    return to_dev(a[:1], dtype, dev).expand(B, N, K)


def run_leaf(kind, case, dtype, dev, layout="rows", want_da=True):
    """One call of the leaf ``kind`` on ``case``: dict of numpy float64 S [B], R [B, K], g0, g1 [B, K, D],
    r [B, N, K] (rows leaves with want_da) -- or S, R, m, G for "mvn"."""
    from pyro_amd import kernels as k

    def host(t):
        return None if t is None else t.detach().double().cpu().numpy()

    if kind == "mvn":
        S, R, m, G = k.mixture_mvn_fwd_bwd(to_dev(case.x, dtype, dev), to_dev(case.a, dtype, dev),
                                           to_dev(case.loc, dtype, dev), to_dev(case.W, dtype, dev))
        return dict(S=host(S), R=host(R), m=host(m), G=host(G))
    K, D = case.K, case.D
    if kind in ("scalar", "rows"):
        assert D == 1
        x = to_dev(case.x[:, 0], dtype, dev)
        f0, s0, b0 = _flat(case.p0, dtype, dev)
        f1, s1, b1 = _flat(case.p1, dtype, dev)
        if kind == "scalar":
            out = k.mixture_fwd_bwd(case.dist_id, x, to_dev(case.a, dtype, dev), f0, s0, f1, s1, b0, b1)
            S, R, g0 = out[:, 0], out[:, 1:1 + K], out[:, 1 + K:1 + 2 * K]
            g1, r = (out[:, 1 + 2 * K:] if f1 is not None else None), None
        else:
            S, r, g0, g1 = k.mixture_rows_fwd_bwd(case.dist_id, x, _row_weights(case.a, layout, dtype, dev), f0, s0,
                                                  f1, s1, b0, b1, want_da=want_da)
            R = None                    # (the rows leaves return r itself, scored per element; no R of their own)
        g0, g1 = g0[..., None], (None if g1 is None else g1[..., None])
    elif kind == "diag":
        assert case.dist_id == NORMAL
        S, R, g0, g1 = k.mixture_diag_normal_fwd_bwd(to_dev(case.x, dtype, dev), to_dev(case.a, dtype, dev),
                                                     to_dev(case.p0, dtype, dev), to_dev(case.p1, dtype, dev))
        r = None
    elif kind == "rows_diag":
        assert case.dist_id == NORMAL
        S, r, g0, g1 = k.mixture_rows_diag_normal_fwd_bwd(to_dev(case.x, dtype, dev),
                                                          _row_weights(case.a, layout, dtype, dev),
                                                          to_dev(case.p0, dtype, dev), to_dev(case.p1, dtype, dev),
                                                          want_da=want_da)
        R = None
    else:
        assert kind == "event"
        S, R, g0, g1 = k.mixture_event_fwd_bwd(case.dist_id, to_dev(case.x, dtype, dev), to_dev(case.a, dtype, dev),
                                               to_dev(case.p0, dtype, dev),
                                               None if case.p1 is None else to_dev(case.p1, dtype, dev))
        r = None
    return dict(S=host(S), R=host(R), g0=host(g0), g1=host(g1), r=host(r))


def same_bits(o1, o2):
    """Two runs' outputs, bit for bit (NaNs included)."""
    return all((o1[q] is None and o2[q] is None) or o1[q].tobytes() == o2[q].tobytes() for q in o1)


def leaf_ks(kind, case, dtype, cus):
    """k of the rule per output of one call."""
    f32 = dtype == F32
    if kind == "mvn":
        return mvn_plan(case.K, case.D, case.B, case.N, f32)["TR"]
    if kind == "event":
        p = event_plan(case.dist_id, case.K, case.D, case.B, case.N, f32)
        return dict(S=p["DC"], R=p["TB"], g0=p["TB"], g1=p["TB"])
    n = lane_plan(case.N, case.K, case.B, cus, 4 if kind in ("scalar", "rows") else 2)["rows_per_lane"]
    return dict(S=n, R=n, g0=n, g1=n, r=0)


# ---- the parent commit's bits ----------------------------------------------------------------------------------------
def bits_cases():
    """kind -> the geometry case whose outputs the kernel fixes must leave bit for bit as the parent commit had them."""
    return {
        "scalar": geometry(NORMAL, 1031, 5, 1, 3, seed=21), "scalar/gamma": geometry(GAMMA, 1031, 5, 1, 3, seed=21),
        "rows": geometry(NORMAL, 1031, 5, 1, 3, rows=True, seed=21),
        "diag": geometry(NORMAL, 1031, 5, 3, 3, seed=21), "rows_diag": geometry(NORMAL, 1031, 5, 3, 3, rows=True, seed=21),
        "event": geometry(NORMAL, 517, 17, 17, 3, seed=21), "event/gamma": geometry(GAMMA, 517, 17, 17, 3, seed=21),
        "event/lognormal": geometry(LOG_NORMAL, 517, 17, 17, 3, seed=21),
        "mvn": mvn_geometry(517, 5, 9, 3, seed=21),
    }


def bits_digest(out):
    """sha256 over the outputs' float64 bytes (-0 counted as 0, as torch.equal does)."""
    import hashlib
    h = hashlib.sha256()
    for q in sorted(out):
        if out[q] is not None:
            h.update(np.ascontiguousarray(out[q] + 0.0).tobytes())
    return h.hexdigest()[:32]


# recorded from the parent commit's library on the MI355X: "<kind> <dtype>" -> bits_digest of run_leaf's outputs
PARENT_BITS = {
    'scalar f32': '996c90693702c056a51e42750ee73c74',
    'scalar/gamma f32': '7f2d76cafacca258bcdbd62427841ba7',
    'rows f32': 'f39a572043b37990ac2605f0e4bdff49',
    'diag f32': '183d4abcf86c15e23841a298d08f18ea',
    'rows_diag f32': '720f9a6f7f97a43c6116e9a7dc201c30',
    'event f32': '701135b7844c3083515c55b06a3b18db',
    'event/gamma f32': '587570d39d30d964bd48f1ea32862f9d',
    'event/lognormal f32': 'dbda7fca1064540d0762e65d33136a94',
    'mvn f32': '166028a250a3d2a3a9f482f5f67f6086',
    'scalar f64': '6d027b95ea1374b3f13d050c832e4067',
    'scalar/gamma f64': '689f6ac8b31daeefff68e54f9635280d',
    'rows f64': '655a3ef214924886a4c254bfa28c5ed0',
    'diag f64': '12b0bedc746798764543974ba0a9b422',
    'rows_diag f64': '7c1ddbcd78a169851f35ac727facdb25',
    'event f64': '7d2d2c7fe9125021f7cfb51f0a770de8',
    'event/gamma f64': '25dbbf3308cedc771138ef40162a615f',
    'event/lognormal f64': '319a6d187ee269adb50cc4b66baf37d0',
    'mvn f64': '123dedf68ffa08ae44be0df8b308bf20',
}
