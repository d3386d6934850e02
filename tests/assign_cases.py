"""Shared pieces of the infer_discrete / mixture_assign tests: float64 torch statements of what kernels.mixture_assign
and kernels.mixture_assign_diag_normal return, small enumerated models with their brute-force joint tables, and the
fixed-seed draws of TraceEnum_ELBO.sample_posterior that tests/golden/sample_posterior_kat.npz records."""
import itertools

import numpy as np
import torch

from tests.event_mixture_cases import FAMILIES, dist_id, family_data, family_params, torch_family

F32_MARGIN, F64_MARGIN = 1e-4, 1e-10


# ---- the kernels' arithmetic in float64 --------------------------------------------------------------------------
def assign_scores(family, x, a, p0, p1):
    """t [B, N, K] in float64: a[b, (n,) k] + log p(x[n] | p0[b, k], p1[b, k]).  x [N] with p0 / p1 [B | 1, K | 1], or
    x [N, D] with p0 / p1 [B | 1, K | 1, D | 1] (the features' log-densities summed); a [B, K] or [B, N, K]."""
    dt = torch.float64
    x = x.detach().to(dt)
    a = a.detach().to(dt)
    q0 = p0.detach().to(dt)
    q1 = None if p1 is None else p1.detach().to(dt)
    if x.dim() == 2:
        lp = torch_family(family, q0[:, None], None if q1 is None else q1[:, None]).log_prob(x[:, None, :]).sum(-1)
    else:
        lp = torch_family(family, q0[:, None, :], None if q1 is None else q1[:, None, :]).log_prob(x[:, None])
    if a.dim() == 2:
        a = a[:, None, :]
    return a + lp                                                               # [B, N, K]


def map_reference(t, margin):
    """(z [B, N] = torch.argmax over k -- 0 for a row with a NaN --, keep [B, N]: rows whose top two scores lie at
    least margin * max(1, |m|) apart, or that have one term only)."""
    nan = torch.isnan(t).any(-1)
    tt = torch.where(nan[..., None], torch.zeros_like(t), t)
    z = torch.argmax(tt, -1)
    if t.shape[-1] == 1:
        return z, torch.ones_like(nan)
    top = torch.topk(tt, 2, dim=-1).values
    m = top[..., 0]
    gap = top[..., 0] - top[..., 1]
    gap = torch.where(torch.isnan(gap), torch.zeros_like(gap), gap)             # (-inf - -inf: a dead row, z = 0)
    keep = (gap > margin * torch.clamp(m.abs(), min=1.0)) | torch.isneginf(m) | nan
    return z, keep


def draw_reference(t, u, margin):
    """Inverse CDF in float64: e = exp(t - max t), c = cumsum(e) in index order, z = the smallest k with
    c_k > u c_{K-1}, clamped to the largest k with e_k > 0; a row with no finite term: 0.  u [B, N].
    -> (z [B, N], keep [B, N]: rows where u c_{K-1} is further than margin * c_{K-1} from every c_k)."""
    K = t.shape[-1]
    u = u.to(torch.float64)
    m = t.max(-1, keepdim=True).values
    dead = (torch.isnan(t).any(-1, keepdim=True) | torch.isneginf(m))
    e = torch.where(dead, torch.zeros_like(t), torch.exp(t - torch.where(dead, torch.zeros_like(m), m)))
    c = torch.cumsum(e, -1)
    total = c[..., -1:]
    thr = u[..., None] * total
    ks = torch.arange(K, device=t.device)
    first = torch.where(c > thr, ks, torch.full_like(ks, K)).min(-1).values
    last = torch.where(e > 0, ks, torch.full_like(ks, -1)).max(-1).values
    z = torch.minimum(first, last).clamp(min=0)
    z = torch.where(dead[..., 0], torch.zeros_like(z), z)
    near = ((c[..., :-1] - thr).abs() <= margin * total).any(-1) if K > 1 else torch.zeros_like(dead[..., 0])
    return z, ~near | dead[..., 0]


def philox_uniforms(B, N, dtype, seed, offset, device="cpu"):
    """[B, N]: element b N + n of the Philox uniform stream (oracle/philox.py), in ``dtype``."""
    from oracle import philox

    np_dt = np.float32 if dtype == torch.float32 else np.float64
    return torch.as_tensor(philox.uniform(B * N, np_dt, seed, offset).reshape(B, N), device=device)


def unflat(p, s, bs, B, K):
    """the [B, K] view of a flat parameter addressed b * bs + k * s (stride 0: shared)"""
    return None if p is None else p.as_strided((B, K), (bs, s))


def kernel_case(family, N, K, B, D=None, layout="shared", share=None, seed=0):
    """float64 CPU inputs of one kernel case: x [N] (D None) or [N, D] drawn from the family's mixture; a: "shared"
    [B, K] log-weights, or [B, N, K] per row ("rows": row-major, "sets": one row-major set for every b, set-stride 0,
    "sliced": K columns of a wider row-major matrix: see lay_out); p0, p1 [B | 1, K | 1(, D)] (p1 None for
    one-parameter families).  ``share``: None, "k" (p1 -- p0 for one-parameter families -- one value for every
    component) or "b" (the parameters one set for every b)."""
    g = torch.Generator().manual_seed(seed)
    d = 1 if D is None else D
    P0, P1 = family_params(family, K, d, g)
    x = family_data(family, P0, P1, N, g)
    Bp = 1 if share == "b" else B
    ps = [family_params(family, K, d, g) for _ in range(Bp)]
    p0 = torch.stack([q[0] for q in ps])
    p1 = None if P1 is None else torch.stack([q[1] for q in ps])
    if share == "k":
        if p1 is None:
            p0 = p0[:, :1]
        else:
            p1 = p1[:, :1]
    if D is None:
        x, p0, p1 = x[:, 0], p0[..., 0], None if p1 is None else p1[..., 0]
    if layout == "shared":
        a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    else:
        Ba = 1 if layout == "sets" else B
        a = torch.log_softmax(1.5 * torch.randn(Ba, N, K, generator=g, dtype=torch.float64), -1)
    return {"x": x, "a": a, "p0": p0.contiguous(), "p1": None if p1 is None else p1.contiguous()}


def lay_out(a, B, layout):
    """a [B, K], or [B | 1, N, K] contiguous -> the view of the requested memory layout ("sliced": the first K of K + 3
    columns: component stride 1, row stride K + 3, read in place)"""
    if a.dim() == 2:
        return a
    if layout == "sliced":
        wide = torch.full((a.shape[0], a.shape[1], a.shape[2] + 3), float("nan"), dtype=a.dtype, device=a.device)
        wide[..., :a.shape[2]] = a
        a = wide[..., :a.shape[2]]
    return a.expand(B, a.shape[1], a.shape[2])


def flat(p, B, K):
    """p [B | 1, K | 1] -> (flat contiguous tensor addressed b * bs + k * s, s, bs): the scalar kernels' convention."""
    if p is None:
        return None, 0, 0
    Bp, Kp = p.shape
    return p.contiguous().reshape(-1), (1 if Kp == K and K > 1 else 0), (Kp if Bp == B and B > 1 else 0)


def standins(calls):
    """float64 torch stand-ins for kernels.mixture_assign / mixture_assign_diag_normal that note every call in
    ``calls`` as (kernel, a's shape, a's strides, mode[, family id])."""
    names = {dist_id(f): f for f in FAMILIES}

    def pick(t, mode, x, seed, offset):
        if mode == 0:
            return map_reference(t, 0.0)[0]
        B, N = t.shape[:2]
        return draw_reference(t, philox_uniforms(B, N, x.dtype, seed, offset), 0.0)[0]

    def scalar(dist, x, a, p0, s0, p1, s1, p0_bs=0, p1_bs=0, mode=0, seed=0, offset=0, offset_dev=None):
        calls.append(("scalar", tuple(a.shape), tuple(a.stride()), int(mode), int(dist)))
        assert x.dim() == 1 and x.is_contiguous() and p0.is_contiguous() and a.dim() in (2, 3)
        B, K = a.shape[0], a.shape[-1]
        assert a.dim() == 2 or a.shape[1] == x.shape[0]
        t = assign_scores(names[int(dist)], x, a, unflat(p0, s0, p0_bs, B, K), unflat(p1, s1, p1_bs, B, K))
        return pick(t, mode, x, seed, offset)

    def diag(x, a, loc, scale, mode=0, seed=0, offset=0, offset_dev=None):
        calls.append(("diag", tuple(a.shape), tuple(a.stride()), int(mode)))
        assert x.dim() == 2 and x.is_contiguous() and loc.is_contiguous() and scale.is_contiguous()
        assert loc.dim() == 3 and scale.dim() == 3 and (a.dim() == 2 or a.shape[1] == x.shape[0])
        return pick(assign_scores("Normal", x, a, loc, scale), mode, x, seed, offset)

    return scalar, diag


# ---- small models and their joint tables ---------------------------------------------------------------------------
def _backend(backend):
    if backend is not None:
        return backend
    import pyro_amd as pyro
    import pyro_amd.distributions as dist

    return pyro, dist


def gmm_tensors(N, K, seed, dtype=torch.float64, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    locs = 2.5 * torch.randn(K, generator=gen, dtype=torch.float64)
    pi = torch.softmax(torch.randn(K, generator=gen, dtype=torch.float64), -1)
    z = torch.randint(0, K, (N,), generator=gen)
    data = locs[z] + 0.8 * torch.randn(N, generator=gen, dtype=torch.float64)
    return {"data": data.to(device, dtype), "pi": pi.to(device, dtype), "locs": (locs + 0.3).to(device, dtype),
            "scale": torch.tensor(0.9, dtype=dtype, device=device)}


def make_gmm(T, backend=None):
    """A plated Gaussian mixture: z enumerated under the data plate; returns z."""
    pyro, dist = _backend(backend)

    def model():
        with pyro.plate("data", T["data"].shape[0]):
            z = pyro.sample("z", dist.Categorical(T["pi"]), infer={"enumerate": "parallel"})
            pyro.sample("obs", dist.Normal(T["locs"][z], T["scale"]), obs=T["data"])
        return z

    return model


def gmm_log_joint(T, z):
    """log p(z, data) [..] of assignments z [.., N] in float64"""
    d = T["data"].double()
    lp = torch.distributions.Normal(T["locs"].double()[z], T["scale"].double()).log_prob(d)
    return (lp + T["pi"].double().log()[z]).sum(-1)


def hmm_tensors(T_len=5, S=3, seed=0, dtype=torch.float64, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)          # noqa: E731
    return {"init": torch.softmax(r(S), -1).to(device, dtype), "tp": torch.softmax(1.5 * r(S, S), -1).to(device, dtype),
            "ep": torch.softmax(1.5 * r(S, 4), -1).to(device, dtype),
            "data": torch.randint(0, 4, (T_len,), generator=gen).to(device)}


def make_hmm(T, backend=None):
    """A pyro.markov chain of len(data) enumerated states with Categorical emissions; returns the list of states."""
    pyro, dist = _backend(backend)

    def model():
        xs = []
        x = None
        for i in pyro.markov(range(T["data"].shape[0])):
            probs = T["init"] if x is None else T["tp"][x]
            x = pyro.sample("x_{}".format(i), dist.Categorical(probs), infer={"enumerate": "parallel"})
            pyro.sample("y_{}".format(i), dist.Categorical(T["ep"][x]), obs=T["data"][i])
            xs.append(x)
        return xs

    return model


def hmm_log_joint(T, xs):
    """log p(x_0.., data) of state sequences xs [.., T] in float64"""
    xs = torch.as_tensor(xs)
    init, tp, ep = T["init"].double().log(), T["tp"].double().log(), T["ep"].double().log()
    lp = init[xs[..., 0]] + ep[xs[..., 0], T["data"][0]]
    for i in range(1, xs.shape[-1]):
        lp = lp + tp[xs[..., i - 1], xs[..., i]] + ep[xs[..., i], T["data"][i]]
    return lp


def global_local_tensors(seed=0, rows=3, vals=3, dtype=torch.float64, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)          # noqa: E731
    return {"ps": torch.tensor(0.35, dtype=dtype, device=device),
            "pi": torch.softmax(r(2, vals), -1).to(device, dtype), "locs": (2.0 * r(vals)).to(device, dtype),
            "shift": torch.tensor(0.7, dtype=dtype, device=device), "data": (1.5 * r(rows)).to(device, dtype)}


def make_global_local(T, backend=None, copies=None):
    """A global Bernoulli site s with a plated Categorical site z (rows x vals of global_local_tensors: 3 rows of 3
    values make 2 x 3^3 joint states) under it.
    ``copies``: an outer plate of that many independent copies of the whole model.  Returns (s, z)."""
    pyro, dist = _backend(backend)
    import contextlib

    def model():
        outer = pyro.plate("copies", copies, dim=-2) if copies else contextlib.nullcontext()
        with outer:
            s = pyro.sample("s", dist.Bernoulli(T["ps"]), infer={"enumerate": "parallel"})
            with pyro.plate("data", T["data"].shape[0], dim=-1):
                z = pyro.sample("z", dist.Categorical(T["pi"][s.long()]), infer={"enumerate": "parallel"})
                pyro.sample("obs", dist.Normal(T["locs"][z] + T["shift"] * s, 1.0), obs=T["data"])
        return s, z

    return model


def global_local_log_joint(T, s, z):
    """log p(s, z, data) of s [..], z [.., rows] in float64"""
    s = torch.as_tensor(s).long()
    z = torch.as_tensor(z)
    ps = T["ps"].double()
    lp = torch.where(s == 1, ps.log(), (1 - ps).log())
    lp = lp + T["pi"].double().log()[s[..., None], z].sum(-1)
    mean = T["locs"].double()[z] + T["shift"].double() * s[..., None]
    return lp + torch.distributions.Normal(mean, 1.0).log_prob(T["data"].double()).sum(-1)


def fitted_mixture(form, device, dtype, N, K, B=3, D=None, family="Normal"):
    """A fitted-style mixture with fixed parameters whose model returns z: ``form`` "plain" (weights shared by the
    rows), "gate" (a gating network's per-row weights), "grouped" (``Categorical(theta[g])``), "sets" (B vectorised
    parameter sets under an outer plate at dim -2), and the forms infer_discrete leaves to its generic route: "mvn"
    (a MultivariateNormal observation), "second" (a second enumerated site in the observation's factor).  Scalar data,
    or D features through ``.to_event(1)``; ``family``: of tests.event_mixture_cases.FAMILIES."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist

    g = torch.Generator().manual_seed(23)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)            # noqa: E731
    d = 1 if D is None else D
    P0, P1 = family_params(family, K, d, g)
    x = family_data(family, P0, P1, N, g)
    sets = [family_params(family, K, d, g) for _ in range(B)]
    p0b = torch.stack([q[0] for q in sets]).to(device, dtype)                   # [B, K, d]
    p1b = None if P1 is None else torch.stack([q[1] for q in sets]).to(device, dtype)
    if D is None:
        x, p0b, p1b = x[:, 0], p0b[..., 0], None if p1b is None else p1b[..., 0]
    x = x.to(device, dtype)
    p0, p1 = p0b[0], None if p1b is None else p1b[0]
    pi = torch.softmax(r(K), -1).to(device, dtype)
    X, W = r(N, 3).to(device, dtype), (0.5 * r(3, K)).to(device, dtype)
    grp, theta = torch.randint(0, 4, (N,), generator=g).to(device), torch.softmax(r(4, K), -1).to(device, dtype)
    rows_b = torch.arange(B, device=device)[:, None]

    def obs_dist(q0, q1):
        if form == "mvn":
            return dist.MultivariateNormal(q0, scale_tril=torch.diag_embed(q1))
        fam = {"Normal": lambda: dist.Normal(q0, q1), "LogNormal": lambda: dist.LogNormal(q0, q1),
               "Exponential": lambda: dist.Exponential(q0), "Bernoulli": lambda: dist.Bernoulli(logits=q0),
               "Poisson": lambda: dist.Poisson(q0), "Gamma": lambda: dist.Gamma(q0, q1)}[family]()
        return fam if D is None else fam.to_event(1)

    def model():
        if form == "sets":
            with pyro.plate("sets", B, dim=-2), pyro.plate("data", N, dim=-1):
                z = pyro.sample("z", dist.Categorical(pi), infer={"enumerate": "parallel"})
                pyro.sample("obs", obs_dist(p0b[rows_b, z], None if p1b is None else p1b[rows_b, z]), obs=x)
            return z
        with pyro.plate("data", N, dim=-1):
            cat = dist.Categorical(logits=X @ W) if form == "gate" else \
                dist.Categorical(theta[grp]) if form == "grouped" else dist.Categorical(pi)
            z = pyro.sample("z", cat, infer={"enumerate": "parallel"})
            q0, q1 = p0[z], None if p1 is None else p1[z]
            if form == "second":
                w = pyro.sample("w", dist.Bernoulli(torch.tensor(0.4, dtype=dtype, device=device)),
                                infer={"enumerate": "parallel"})
                q0 = q0 + (w if D is None else w.unsqueeze(-1))
            pyro.sample("obs", obs_dist(q0, q1), obs=x)
        return z

    return model


def all_configs(sizes):
    return torch.tensor(list(itertools.product(*(range(s) for s in sizes))))


# ---- TraceEnum_ELBO.sample_posterior at a fixed seed (recorded before infer_discrete shared its machinery) ----------
def sample_posterior_draws(n=64):
    """The draws of the sample_posterior cases of tests/posterior_kat_cases.py (run_backwardsample_2, _3 and
    _hmm_joint) on the CPU in float64 at seed 11, n rows each: {name: int64 array}."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd.infer import TraceEnum_ELBO, config_enumerate

    dt = torch.float64
    f = lambda v: torch.tensor(v, dtype=dt)                                      # noqa: E731

    @config_enumerate
    def model2(data):
        with pyro.plate("particles", n):
            x = pyro.sample("x", dist.Categorical(f([0.5, 0.5])))
            z = pyro.sample("z", dist.Bernoulli(f([0.1, 0.9])[x]), obs=data)
        return x, z

    @config_enumerate
    def model3(data):
        with pyro.plate("particles", n):
            p_z = f([[0.9, 0.1], [0.1, 0.9]])
            x = pyro.sample("x", dist.Categorical(f([0.5, 0.5])))
            y = pyro.sample("y", dist.Categorical(f([0.5, 0.5])))
            z = pyro.sample("z", dist.Bernoulli(p_z[x, y]), obs=data)
        return x, y, z

    tp = f([[0.75, 0.25], [0.25, 0.75]])
    ep = f([[0.75, 0.25], [0.25, 0.75]])
    obs = torch.tensor([0, 1, 1, 0])

    @config_enumerate
    def model_hmm(data):
        with pyro.plate("draws", n):
            x = torch.zeros(n, dtype=torch.long)
            xs = []
            for i in pyro.markov(range(4)):
                x = pyro.sample("x_{}".format(i), dist.Categorical(tp[x]))
                pyro.sample("y_{}".format(i), dist.Categorical(ep[x]), obs=data[i].expand(n))
                xs.append(x)
        return xs

    def guide(data):
        pass

    out = {}
    elbo = TraceEnum_ELBO(max_plate_nesting=1)
    pyro.set_rng_seed(11)
    x, _ = elbo.sample_posterior(model2, guide, data=torch.zeros(n, dtype=dt))
    out["bs2/x"] = x.reshape(n).numpy()
    x, y, _ = elbo.sample_posterior(model3, guide, data=torch.ones(n, dtype=dt))
    out["bs3/x"], out["bs3/y"] = x.reshape(n).numpy(), y.reshape(n).numpy()
    xs = elbo.sample_posterior(model_hmm, guide, obs)
    out["hmm/xs"] = torch.stack([v.reshape(n) for v in xs]).numpy()
    return out
