"""Shared pieces of the event-shaped mixture tests: a float64 torch statement of what pa_mixture_event_fwd_bwd returns,
and an enumerated mixture model ``Fam(p0[z], p1[z]).to_event(1)`` for every family of the leaf, in its accepted and
rejected forms."""
import torch

FAMILIES = ("Normal", "LogNormal", "Exponential", "Bernoulli", "Poisson", "Gamma")
TWO_PARAMETERS = ("Normal", "LogNormal", "Gamma")


def dist_id(family):
    from pyro_amd import _lib

    return {"Normal": _lib.DIST_NORMAL, "LogNormal": _lib.DIST_LOG_NORMAL, "Exponential": _lib.DIST_EXPONENTIAL,
            "Bernoulli": _lib.DIST_BERNOULLI_LOGITS, "Poisson": _lib.DIST_POISSON, "Gamma": _lib.DIST_GAMMA}[family]


def torch_family(family, p0, p1):
    """torch.distributions' own family (validation off) over the leaf's parameters (Bernoulli: p0 = logits)."""
    D = torch.distributions
    if family == "Normal":
        return D.Normal(p0, p1, validate_args=False)
    if family == "LogNormal":
        return D.LogNormal(p0, p1, validate_args=False)
    if family == "Exponential":
        return D.Exponential(p0, validate_args=False)
    if family == "Bernoulli":
        return D.Bernoulli(logits=p0, validate_args=False)
    if family == "Poisson":
        return D.Poisson(p0, validate_args=False)
    return D.Gamma(p0, p1, validate_args=False)


def event_leaf_reference(family, x, a, p0, p1, dtype=torch.float64):
    """torch in ``dtype`` (float64 by default): (S [B], dS/da [B, K], dS/dp0 [B, K, D], dS/dp1 [B, K, D] or None) of
    kernels.mixture_event_fwd_bwd -- the same arguments (x [N, D]; a [B, K]; p0 / p1 [B | 1, K | 1, D | 1]).  The
    gradients are per (b, k, d) (a shared parameter's is the sum over its broadcast axes); a row whose logsumexp is
    -inf has no responsibilities."""
    B, K = a.shape
    N, D = x.shape
    with torch.enable_grad():                 # (also when called inside an autograd Function's forward)
        x = x.detach().to(dtype)
        a = a.detach().to(dtype).clone().requires_grad_()
        q0 = p0.detach().to(dtype).expand(B, K, D).clone().requires_grad_()
        q1 = None if p1 is None else p1.detach().to(dtype).expand(B, K, D).clone().requires_grad_()
        lp = torch_family(family, q0[:, :, None, :], None if q1 is None else q1[:, :, None, :]).log_prob(x).sum(-1)
        t = a[:, :, None] + lp                                                   # [B, K, N]
        lse = torch.logsumexp(t.detach(), 1)                                     # [B, N]
        r = torch.exp(t.detach() - lse[:, None])
        r = torch.where(torch.isneginf(lse)[:, None], torch.zeros_like(r), r)
        # d S / d theta = sum_{n, k} r_nk d t_nk / d theta
        params = [a, q0] + ([q1] if q1 is not None else [])
        grads = torch.autograd.grad((r * t).sum(), params)
    return (lse.sum(-1), grads[0], grads[1], grads[2] if q1 is not None else None)


def family_params(family, K, D, gen, confident=False):
    """float64 (p0 [K, D], p1 [K, D] or None) in the family's support."""
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)            # noqa: E731
    n = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)           # noqa: E731
    if family == "Normal":
        return 2.0 * n(K, D), 0.5 + u(K, D)
    if family == "LogNormal":
        return 0.5 * n(K, D), 0.3 + 0.5 * u(K, D)
    if family == "Exponential":
        return 0.3 + 3.0 * u(K, D), None
    if family == "Bernoulli":
        return (40.0 * u(K, D) - 20.0) if confident else 3.0 * n(K, D), None
    if family == "Poisson":
        return 0.5 + 8.0 * u(K, D), None
    return 1.0 + 4.0 * u(K, D), 0.5 + 2.0 * u(K, D)


def family_data(family, p0, p1, N, gen):
    """float64 data [N, D] drawn from the mixture of the components (p0[k], p1[k]) with equal weights."""
    K = p0.shape[0]
    z = torch.randint(0, K, (N,), generator=gen)
    q0 = p0[z]
    q1 = None if p1 is None else p1[z]
    torch.manual_seed(int(torch.randint(0, 2**31, (1,), generator=gen)))
    return torch_family(family, q0, q1).sample().to(torch.float64)


def make_mixture(family, N, K, D, dtype, device, form="plain", subsample_size=None, seed=0):
    """(model, guide, x): Dirichlet weights (a Delta guide), per-component parameters of ``family`` as parameters of
    the model, the assignment enumerated under the data plate and the observation ``Fam(p0[z], p1[z]).to_event(1)``
    over D features.  ``form``: "plain"; "probs" (Bernoulli(probs=probs[z])); "shared_d" (p0 one value per component,
    broadcast over the features); "shared_k" (p1 one row for every component; two-parameter families); "particles"
    (a weight draw per vectorised particle); and the forms the leaf must leave to the generic path: "mask",
    "per_row" (p0 varies along the data plate), "row_weights", "value_grad"."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from torch.distributions import constraints

    gen = torch.Generator().manual_seed(seed)
    P0, P1 = family_params(family, K, D, gen)
    x = family_data(family, P0, P1, N, gen).to(device, dtype)
    P0, P1 = family_params(family, K, D, gen)             # (the model starts away from the data's parameters)
    if form == "shared_d":
        P0 = P0[:, :1]
    positive = family in ("Exponential", "Poisson", "Gamma")
    c0 = constraints.positive if positive else constraints.real
    if form == "probs":
        P0, c0 = torch.sigmoid(P0), constraints.unit_interval
    P0, P1 = P0.to(device, dtype), None if P1 is None else P1.to(device, dtype)
    if form == "shared_k":
        P1 = P1[0]
    if form == "per_row":
        f0 = (1.0 + 0.01 * torch.rand(N, D, generator=gen, dtype=torch.float64)).to(device, dtype)
    if form == "row_weights":
        rw0 = (torch.rand(N, K, generator=gen, dtype=torch.float64) + 0.5).to(device, dtype)
    if form == "mask":
        mask0 = (torch.rand(N, generator=gen) > 0.2).to(device)
    if form == "value_grad":
        x = x.clone().requires_grad_()

    def obs_dist(p0, p1):
        if family == "Normal":
            return dist.Normal(p0, p1)
        if family == "LogNormal":
            return dist.LogNormal(p0, p1)
        if family == "Exponential":
            return dist.Exponential(p0)
        if family == "Bernoulli":
            return dist.Bernoulli(probs=p0) if form == "probs" else dist.Bernoulli(logits=p0)
        if family == "Poisson":
            return dist.Poisson(p0)
        return dist.Gamma(p0, p1)

    def model(x):
        w = pyro.sample("w", dist.Dirichlet(torch.ones(K, dtype=dtype, device=device)))
        p0 = pyro.param("p0", P0.clone(), constraint=c0)
        p1 = None if P1 is None else pyro.param("p1", P1.clone(), constraint=constraints.positive)
        with pyro.plate("data", N, subsample_size=subsample_size) as idx:
            xs = x[idx] if subsample_size is not None else x
            probs = w
            if form == "row_weights":
                rw = pyro.param("row_weights", rw0.clone(), constraint=constraints.positive)
                probs = w * (rw[idx] if subsample_size is not None else rw)
            z = pyro.sample("z", dist.Categorical(probs), infer={"enumerate": "parallel"})
            q0 = p0[z]
            if form == "per_row":
                q0 = q0 * (f0[idx] if subsample_size is not None else f0)
            q1 = None if p1 is None else (p1 if form == "shared_k" else p1[z])
            d = obs_dist(q0, q1)
            if form == "shared_d":
                d = d.expand(d.batch_shape[:-1] + (D,))
            d = d.to_event(1)
            if form == "mask":
                with poutine.mask(mask=mask0):
                    pyro.sample("x", d, obs=xs)
            else:
                pyro.sample("x", d, obs=xs)

    def guide(x):
        if form == "particles":      # a weight draw per particle: the leaf's parameter sets differ
            qc = pyro.param("qc", torch.full((K,), 2.0, dtype=dtype, device=device), constraint=constraints.positive)
            pyro.sample("w", dist.Dirichlet(qc))
            return
        qw = pyro.param("qw", torch.full((K,), 1.0 / K, dtype=dtype, device=device), constraint=constraints.simplex)
        pyro.sample("w", dist.Delta(qw, event_dim=1))

    return model, guide, x
