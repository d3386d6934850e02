"""The per-family arithmetic of csrc/dist_fam.h at the edges of its range -- overflow, underflow,
support boundaries, NaN / inf operands -- through every kernel entry point that evaluates it, against
float64 torch (tests/dist_edge_cases.py: grids, reference, and the one tolerance rule)."""
import numpy as np
import pytest
import torch

from tests import dist_edge_cases as ec

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _k():
    from pyro_amd import kernels
    return kernels


class Case:
    """One family's grid in one precision: the rounded inputs, torch in f64 (and f32), and M."""

    def __init__(self, dist_id, dtype, pts=None):
        self.dist_id, self.dtype = dist_id, dtype
        self.f32 = dtype == torch.float32
        self.v, self.a, self.b = pts if pts is not None else ec.grid(dist_id, self.f32)
        self.n = self.v.size
        self.two = dist_id in ec.TWO_PARAM
        self.r64 = ec.reference(dist_id, self.v, self.a, self.b, torch.float64)
        self.r32 = ec.reference(dist_id, self.v, self.a, self.b, torch.float32) if self.f32 else None
        self.M = ec.magnitude(dist_id, self.v, self.a, self.b)
        self.nan_ok = ec.kept_nan(dist_id, "lp", self.v, self.a, self.b)

    def t(self, x, shape, dev):
        return torch.tensor(x, dtype=self.dtype, device=dev).reshape(shape)

    def ref32(self, what):
        return None if self.r32 is None else self.r32[what]

    def scored(self, what):
        """elements the rule scores, as a bool mask (f32: torch-f32 finite; f64: all)."""
        return np.isfinite(self.r32[what]) if self.f32 else np.ones(self.n, dtype=bool)

    def check(self, what, got, ref64, M, ref32=None, nan_ok=None, inputs=None):
        ec.check("%s %s %s" % (ec.NAMES[self.dist_id], self.dtype, what), got, ref64, M, self.f32,
                 ref32, inputs if inputs is not None else (self.v, self.a, self.b), nan_ok)


def _f32(x):
    """a float64 sum of f32 values as an f32 result holds it (inf where it overflows f32)"""
    with np.errstate(over="ignore"):
        return np.float32(x).astype(np.float64)


def _mask(rng, shape):
    m = rng.uniform(size=shape) < 0.7
    m[..., 0] = True
    return m


# ---- dist.hip: element-wise log_prob, fused masked sums, gradients -------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist_id", sorted(ec.NAMES))
def test_dist_kernels_at_the_edges(gpu, dist_id, dtype):
    k = _k()
    c = Case(dist_id, dtype)
    n, rng = c.n, np.random.default_rng(dist_id)
    # element-wise on a [1, n] frame
    tb = c.t(c.b, (1, n), gpu) if c.two else None
    lp = k.dist_log_prob(dist_id, c.t(c.v, (1, n), gpu), c.t(c.a, (1, n), gpu), tb, 1, n)
    c.check("log_prob", lp.cpu().numpy(), c.r64["lp"], c.M["lp"], c.ref32("lp"), c.nan_ok)
    # gradients on a [n, 3] frame of column-broadcast operands, masked, scale 0.5, row weights 2^j
    tv, ta = c.t(c.v, (n, 1), gpu), c.t(c.a, (n, 1), gpu)
    tb = c.t(c.b, (n, 1), gpu) if c.two else None
    m = _mask(rng, (n, 3))
    w = np.array([1.0, -2.0, 0.25, 4.0])[np.arange(n) % 4][:, None]
    outs = k.dist_log_prob_grad(dist_id, c.t(w, (n, 1), gpu), tv, ta, tb, torch.tensor(m, device=gpu),
                                0.5, n, 3, (True, True, c.two))
    for name, o in zip(("dv", "da", "db"), outs):
        if o is None:
            continue
        f = lambda x: np.where(m, 0.5 * w * x[:, None], 0.0)   # noqa: E731
        r32 = None if c.r32 is None else _f32(f(c.r32[name]))
        c.check(name, o.cpu().numpy(), f(c.r64[name]), np.abs(f(c.M[name])), r32,
                inputs=[np.broadcast_to(x[:, None], (n, 3)) for x in (c.v, c.a, c.b)])
    # fused masked sums: few columns (one workgroup) and many (the partial-sum path)
    for cols in (3, 1031):
        m = _mask(rng, (n, cols))
        if c.f32:
            m &= c.scored("lp")[:, None]       # rows torch-f32 cannot score are masked out
        cnt = m.sum(1)
        s, tot = k.dist_log_prob_sum(dist_id, tv, ta, tb, torch.tensor(m, device=gpu), 0.5, n, cols,
                                     want_total=True)
        with np.errstate(all="ignore"):
            f = lambda x: np.where(cnt > 0, 0.5 * cnt * x, 0.0)   # noqa: E731
            r64, M = f(c.r64["lp"]), np.abs(f(c.M["lp"]))
            r32 = None if c.r32 is None else _f32(f(c.r32["lp"]))
            nan_ok = c.nan_ok & (cnt > 0)
            c.check("row sums of %d" % cols, s.cpu().numpy(), r64, M, r32, nan_ok)
            kept = ~(nan_ok & np.isnan(s.cpu().numpy()))
            c.check("total of %d" % cols, tot.item(), r64[kept].sum(), M[kept].sum(),
                    None if r32 is None else _f32(r32[kept].sum()), inputs=())


# ---- dist_nd.hip: one broadcast operand ---------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist_id", sorted(ec.NAMES))
def test_dist_nd_kernels_at_the_edges(gpu, dist_id, dtype):
    k = _k()
    c = Case(dist_id, dtype)
    n, rng = c.n, np.random.default_rng(100 + dist_id)
    shape = (2, n)
    tv = c.t(np.stack([c.v, c.v]), shape, gpu)
    ta = c.t(c.a, (1, n), gpu)                       # broadcast over the leading dimension
    tb = c.t(np.stack([c.b, c.b]), shape, gpu) if c.two else None
    # the sum over the elements with a finite reference (the rest masked out)
    m = _mask(rng, shape) & np.isfinite(c.r64["lp"]) & c.scored("lp")
    tot = k.dist_log_prob_sum_nd(dist_id, shape, tv, ta, tb, torch.tensor(m, device=gpu), 1.5)
    cnt = m.sum(0)
    r32 = None if c.r32 is None else _f32((1.5 * cnt * np.where(cnt > 0, c.r32["lp"], 0)).sum())
    c.check("nd sum", tot.item(), (1.5 * cnt * np.where(cnt > 0, c.r64["lp"], 0)).sum(),
            (1.5 * cnt * np.where(cnt > 0, c.M["lp"], 0)).sum(), r32, inputs=())
    # gradients of every element, masked (upstream 4, scale 0.5: exact weights)
    m = _mask(rng, shape)
    g = torch.tensor([4.0], dtype=dtype, device=gpu)
    outs = k.dist_log_prob_grad_nd(dist_id, shape, g, tv, ta, tb, torch.tensor(m, device=gpu), 0.5,
                                   (True, True, c.two))
    for name, o in zip(("dv", "da", "db"), outs):
        if o is None:
            continue
        f = lambda x: np.where(m, 2.0 * x[None, :], 0.0)   # noqa: E731
        c.check("nd " + name, o.cpu().numpy(), f(c.r64[name]), np.abs(f(c.M[name])),
                None if c.r32 is None else _f32(f(c.r32[name])),
                inputs=[np.broadcast_to(x, shape) for x in (c.v, c.a, c.b)])


# ---- multisite: every family in one launch --------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_multisite_at_the_edges(gpu, dtype):
    k = _k()
    rng = np.random.default_rng(7)
    cases = [Case(d, dtype) for d in sorted(ec.NAMES)]
    coefs = [0.5, 2.0, 1.0, 0.25] * 3
    for finite_only in (True, False):
        entries, masks = [], []
        for c, coef in zip(cases, coefs):
            m = _mask(rng, (1, c.n))[0]
            if finite_only:                  # the total is scored: non-finite elements masked out
                m &= np.isfinite(c.r64["lp"]) & c.scored("lp")
            masks.append(m)
            entries.append(dict(dist=c.dist_id, rows=1, cols=c.n, value=c.t(c.v, (1, c.n), gpu),
                                p0=c.t(c.a, (1, c.n), gpu),
                                p1=c.t(c.b, (1, c.n), gpu) if c.two else None,
                                mask=torch.tensor(m[None, :], device=gpu), coef=coef,
                                need=(True, True, c.two)))
        tot, grads = k.multi_log_prob_sum_grad(entries, 2.0, dtype, gpu)
        if finite_only:
            parts = [(2 * coef * np.where(m, c.r64["lp"], 0).sum(), 2 * coef * np.where(m, c.M["lp"], 0).sum(),
                      0 if c.r32 is None else 2 * coef * np.where(m, c.r32["lp"], 0).sum())
                     for c, coef, m in zip(cases, coefs, masks)]
            r64, M, r32 = (sum(p[j] for p in parts) for j in range(3))
            cases[0].check("multisite total", tot.item(), r64, M, _f32(r32) if cases[0].f32 else None, inputs=())
        for c, coef, m, gr in zip(cases, coefs, masks, grads):
            for name, o in zip(("dv", "da", "db"), gr):
                if o is None:
                    continue
                f = lambda x: np.where(m, 2 * coef * x, 0.0)   # noqa: E731
                c.check("multisite " + name, o.cpu().numpy().ravel(), f(c.r64[name]), np.abs(f(c.M[name])),
                        None if c.r32 is None else _f32(f(c.r32[name])))


# ---- mixture.hip: the enumerated mixture leaf -------------------------------------------------------

# (p0 [K], p1 [K] or None, live x values, a value outside every component's support or None)
MIXTURES = {
    0: ([0.0, 1e6, -3.0], [1e-6, 1.0, 1e6], [0.0, 1e-6, 3.0, -1e6, 1e12, 1e30], np.inf),
    3: ([0.0, 40.0, -5.0], [1e-3, 1.0, 1e3], [1e-30, 1e-6, 1.0, 2.5, 1e17, 1e30], np.inf),
    4: ([1e-30, 1.0, 1e10], None, [0.0, 1e-30, 1.0, 1e20], np.inf),
    1: ([-1e30, -17.0, 1e-8, 40.0, 1e30], None, [0.0, 1.0, 0.0, 1.0], None),
    8: ([1e-30, 1.0, 1e6, 1e9], None, [0.0, 1.0, 1e6, 1e9], -1.0),
    6: ([1e-3, 0.5, 0.999], [1e-10, 1.0, 1e10], [1e-30, 1e-6, 1.0, 1e6, 1e30], np.inf),
}


def _mixture_ref(dist_id, x, lw, p0, p1, dtype):
    """S, dS/dlogw, dS/dp0, dS/dp1 (numpy f64) of torch in ``dtype``; rows whose every term is -inf
    contribute S = -inf and no gradient (the convention of test_logsumexp_terms_nan_and_inf_follow_torch)."""
    t = lambda z: torch.tensor(z, dtype=dtype, requires_grad=True)   # noqa: E731
    tw, t0 = t(lw), t(p0)
    t1 = t(p1 if p1 is not None else np.zeros(len(p0)))
    tx = torch.tensor(x, dtype=dtype)
    with torch.no_grad():
        dead = ~((tw[:, None] + ec.torch_log_prob(dist_id, tx[None, :], t0[:, None], t1[:, None])).max(0).values
                 > -np.inf)
    terms = tw[:, None] + ec.torch_log_prob(dist_id, tx[None, ~dead], t0[:, None], t1[:, None])
    S = torch.logsumexp(terms, 0).sum()
    gs = torch.autograd.grad(S, [tw, t0, t1], allow_unused=True)
    gs = [torch.zeros_like(tw) if g is None else g for g in gs]
    S = S.item() if not dead.any() else -np.inf
    return [S] + [g.double().numpy() for g in gs]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist_id", sorted(MIXTURES))
def test_mixture_leaf_at_the_edges(gpu, dist_id, dtype):
    k = _k()
    f32 = dtype == torch.float32
    p0, p1, xs, out = MIXTURES[dist_id]
    K = len(p0)
    lw = np.log(np.arange(1, K + 1) / (K * (K + 1) / 2))
    rnd = lambda z: None if z is None else np.asarray(z, np.float64).astype(np.float32 if f32 else np.float64).astype(np.float64)  # noqa: E731
    p0, p1, lw = rnd(p0), rnd(p1), rnd(lw)
    for with_out in ((False, True) if out is not None else (False,)):
        x = rnd(xs + ([out] if with_out else []))
        ref = _mixture_ref(dist_id, x, lw, p0, p1, torch.float64)
        r32 = _mixture_ref(dist_id, x, lw, p0, p1, torch.float32) if f32 else None
        # M: the terms' magnitudes weighted by the responsibilities
        pb0, pb1 = p0[:, None], (p1 if p1 is not None else np.zeros(K))[:, None]
        xb = np.broadcast_to(x[None, :], (K, x.size))
        Mt = ec.magnitude(dist_id, xb, pb0, pb1)
        with np.errstate(all="ignore"):
            lp = ec.reference(dist_id, xb.ravel(), np.broadcast_to(pb0, xb.shape).ravel(),
                              np.broadcast_to(pb1, xb.shape).ravel())
            terms = lw[:, None] + lp["lp"].reshape(K, -1)
            live = np.isfinite(terms).any(0)
            r = np.where(live, np.exp(terms - np.where(live, terms.max(0), 0)), 0.0)
            r = r / np.where(live, r.sum(0), 1.0)
            Mterm = np.abs(lw)[:, None] + Mt["lp"]
            Mrow = (r * Mterm).sum(0) + 1
            Mr = np.where(r > 0, Mterm + Mrow, 0.0)       # the error of a responsibility, relative
            M_S = Mrow[live].sum()
            M_a = (r * (1 + Mr)).sum(1)
            M_g = [np.where(r > 0, r * (np.abs(Mt[q]) + np.abs(lp[q].reshape(K, -1)) * Mr), 0).sum(1)
                   for q in ("da", "db")]
        tx = torch.tensor(x, dtype=dtype, device=gpu)
        to = lambda z: None if z is None else torch.tensor(z, dtype=dtype, device=gpu)   # noqa: E731
        got = k.mixture_fwd_bwd(dist_id, tx, to(lw), to(p0), 1, to(p1), 1).cpu().numpy()
        what = "%s mixture%s %s" % (ec.NAMES[dist_id], " with an impossible row" if with_out else "", dtype)
        ec.check(what + " S", got[0], ref[0], M_S, f32, None if r32 is None else r32[0], inputs=())
        for j, (name, M) in enumerate((("dlogw", M_a), ("dp0", M_g[0]), ("dp1", M_g[1]))):
            if name == "dp1" and p1 is None:
                continue
            ec.check(what + " " + name, got[1 + j * K:1 + (j + 1) * K], ref[1 + j], M, f32,
                     None if r32 is None else r32[1 + j], inputs=())


# ---- dirichlet.hip -----------------------------------------------------------------------------------

def _dirichlet_case(K, rows, f32):
    conc = np.array([1e-3, 0.5, 1.0, 3.0, 1e5])
    c = conc[(np.arange(rows)[:, None] + np.arange(K)[None, :]) % conc.size].astype(np.float64)
    x = np.empty((rows, K))
    for r in range(rows):
        if r % 2 == 0:                          # near a vertex
            d = 1e-30
            x[r] = d
            x[r, r % K] = 1 - (K - 1) * d
        else:
            x[r] = np.arange(1, K + 1) / (K * (K + 1) / 2)
    if K == 2:                                  # exactly on the boundary, where c == 1 there
        x[1], c[1] = [0.0, 1.0], [1.0, 3.0]
    if f32:
        x, c = x.astype(np.float32).astype(np.float64), c.astype(np.float32).astype(np.float64)
    return x, c


def _dirichlet_ref(x, c, w, dtype):
    tx, tc = (torch.tensor(z, dtype=dtype, requires_grad=True) for z in (x, c))
    lp = torch.distributions.Dirichlet(tc, validate_args=False).log_prob(tx)
    gx, gc = torch.autograd.grad((lp * torch.tensor(w, dtype=dtype)).sum(), [tx, tc])
    return lp.detach().double().numpy(), gx.double().numpy(), gc.double().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,rows", [(2, 64), (1024, 6), (5000, 2)])
def test_dirichlet_at_the_edges(gpu, K, rows, dtype):
    k = _k()
    f32 = dtype == torch.float32
    x, c = _dirichlet_case(K, rows, f32)
    w = np.array([1.0, -0.5, 2.0])[np.arange(rows) % 3]
    ref = _dirichlet_ref(x, c, w, torch.float64)
    r32 = _dirichlet_ref(x, c, w, torch.float32) if f32 else (None, None, None)
    with np.errstate(all="ignore"):
        cm1 = np.where(c == 1, 0.0, np.abs(c) + 1)
        cs = c.sum(1)
        M_lp = (cm1 * np.where(cm1 == 0, 0, np.abs(np.log(x)))).sum(1) + ec._lgM(cs) + ec._lgM(c).sum(1)
        M_dx = np.abs(w)[:, None] * cm1 / x
        M_dc = np.abs(w)[:, None] * (np.where(c == 1, 0, np.abs(np.log(x))) + ec._psiM(cs)[:, None] + ec._psiM(c))
    tx, tc = (torch.tensor(z, dtype=dtype, device=gpu) for z in (x, c))
    lp = k.dirichlet_log_prob(tx, tc).cpu().numpy()
    dx, dc = k.dirichlet_log_prob_grad(torch.tensor(w, dtype=dtype, device=gpu), tx, tc, True, True)
    what = "Dirichlet K=%d %s " % (K, dtype)
    ec.check(what + "log_prob", lp, ref[0], M_lp, f32, r32[0], inputs=())
    ec.check(what + "dx", dx.cpu().numpy(), ref[1], M_dx, f32, r32[1], inputs=())
    ec.check(what + "dc", dc.cpu().numpy(), ref[2], M_dc, f32, r32[2], inputs=())


# ---- the class route users call --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist_id,name", [(2, "HalfCauchy"), (5, "HalfNormal"), (7, "Beta"), (6, "Gamma"),
                                           (9, "Binomial")])
def test_distribution_classes_at_the_edges(gpu, dist_id, name, dtype):
    import pyro_amd.distributions as d
    c = Case(dist_id, dtype)
    req = (dist_id != 9, True, dist_id in (6, 7))       # Binomial: the logits only
    tv, ta, tb = (torch.tensor(z, dtype=dtype, device=gpu, requires_grad=q) for z, q in zip((c.v, c.a, c.b), req))
    dd = {2: lambda: d.HalfCauchy(ta, validate_args=False), 5: lambda: d.HalfNormal(ta, validate_args=False),
          7: lambda: d.Beta(ta, tb, validate_args=False), 6: lambda: d.Gamma(ta, tb, validate_args=False),
          9: lambda: d.Binomial(tb, logits=ta, validate_args=False)}[dist_id]()
    lp = dd.log_prob(tv)
    c.check("class log_prob", lp.detach().cpu().numpy(), c.r64["lp"], c.M["lp"], c.ref32("lp"), c.nan_ok)
    ins = [(nm, t) for nm, t, q in zip(("dv", "da", "db"), (tv, ta, tb), req) if q]
    gs = torch.autograd.grad(lp.sum(), [t for _, t in ins])
    for (nm, _), g in zip(ins, gs):
        c.check("class " + nm, g.cpu().numpy(), c.r64[nm], c.M[nm], c.ref32(nm))


# ---- the two KL pieces against torch's kl_divergence ------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_kl_pieces_sum_to_minus_torch_kl(gpu, dtype):
    k = _k()
    f32 = dtype == torch.float32
    lq, sq, lp, sp = ec._prod([0.0, 3.0, -1e6], [1e-30, 1e-6, 1.0, 1e6], [0.5, -2e6], [1e-6, 1.0, 1e6, 1e30])
    if f32:
        lq, sq, lp, sp = (z.astype(np.float32).astype(np.float64) for z in (lq, sq, lp, sp))
    n = lq.size

    def ref(dt):
        ts = [torch.tensor(z, dtype=dt, requires_grad=True) for z in (lq, sq, lp, sp)]
        D = torch.distributions
        out = -D.kl_divergence(D.Normal(ts[0], ts[1]), D.Normal(ts[2], ts[3]))
        return [out.detach().double().numpy()] + [g.double().numpy() for g in torch.autograd.grad(out.sum(), ts)]
    r64, r32 = ref(torch.float64), (ref(torch.float32) if f32 else [None] * 5)
    m10, m11 = ec.magnitude(10, lq, lp, sp), ec.magnitude(11, sq, sp, sp)
    t = lambda z: torch.tensor(z, dtype=dtype, device=gpu).reshape(1, n)   # noqa: E731
    one = torch.ones((1, 1), dtype=dtype, device=gpu)
    l10 = k.dist_log_prob(10, t(lq), t(lp), t(sp), 1, n).cpu().numpy().ravel()
    l11 = k.dist_log_prob(11, t(sq), t(sp), None, 1, n).cpu().numpy().ravel()
    g10 = [o.cpu().numpy().ravel() for o in k.dist_log_prob_grad(10, one, t(lq), t(lp), t(sp), None, 1.0, 1, n,
                                                                   (True, True, True))]
    g11 = [o.cpu().numpy().ravel() for o in k.dist_log_prob_grad(11, one, t(sq), t(sp), None, None, 1.0, 1, n,
                                                                   (True, True, False))[:2]]
    ins = (lq, sq, lp, sp)
    ec.check("KL %s" % dtype, l10 + l11, r64[0], m10["lp"] + m11["lp"], f32, r32[0], ins)
    for j, (got, M) in enumerate(((g10[0], m10["dv"]), (g11[0], m11["dv"]), (g10[1], m10["da"]),
                                  (g10[2] + g11[1], m10["db"] + m11["da"]))):
        ec.check("KL %s d%d" % (dtype, j), got, r64[1 + j], M, f32, r32[1 + j], ins)


# ---- f32 scales below the normal range ----------------------------------------------------------------------

_DENORMAL_XFAIL = pytest.mark.xfail(strict=True, reason="pos_log / pos_rcp (the hardware log and reciprocal of the "
                                   "f32 Normal hot path) are documented for normal-range scales only")


@pytest.mark.parametrize("dist_id", [pytest.param(10, marks=_DENORMAL_XFAIL), pytest.param(11, marks=_DENORMAL_XFAIL)])
def test_f32_denormal_scales(gpu, dist_id):
    """f32 scales below 2^-126.  (Normal itself is not listed: torch-f32 squares the scale first, so its
    own result is non-finite there and the rule scores nothing.)"""
    k = _k()
    c = Case(dist_id, torch.float32, ec.denormal_grid(dist_id))
    n = c.n
    tb = c.t(c.b, (1, n), gpu) if c.two else None
    tv, ta = c.t(c.v, (1, n), gpu), c.t(c.a, (1, n), gpu)
    lp = k.dist_log_prob(dist_id, tv, ta, tb, 1, n)
    c.check("denormal log_prob", lp.cpu().numpy(), c.r64["lp"], c.M["lp"], c.ref32("lp"))
    one = torch.ones((1, 1), dtype=torch.float32, device=gpu)
    outs = k.dist_log_prob_grad(dist_id, one, tv, ta, tb, None, 1.0, 1, n, (True, True, c.two))
    for name, o in zip(("dv", "da", "db"), outs):
        if o is not None:
            c.check("denormal " + name, o.cpu().numpy(), c.r64[name], c.M[name], c.ref32(name))
