"""Shared pieces of the per-row-weights mixture tests: a float64 torch statement of what kernels.mixture_rows_fwd_bwd and
kernels.mixture_rows_diag_normal_fwd_bwd return, and enumerated mixture models whose assignment probabilities differ
from row to row, in the forms the leaf accepts and the forms that must stay on the generic path."""
import torch

from tests.event_mixture_cases import family_data, family_params, torch_family

ACCEPTED = ("experts", "grouped", "labels", "particles", "subsample", "detached")
REJECTED = ("event", "mvn", "per_row", "mask", "value_grad")


def row_leaf_reference(family, x, a, p0, p1, dtype=torch.float64):
    """torch in ``dtype`` (float64 by default): (S [B], dS/da [B, N, K], dS/dp0, dS/dp1 or None) of the per-row leaf.
    x [N] with p0 / p1 [B | 1, K | 1] (scalar observations), or x [N, D] with p0 / p1 [B | 1, K | 1, D | 1] (the
    features' log-densities summed inside the logsumexp); a [B, N, K], any view.  The parameter gradients are per
    (b, k[, d]) -- a shared parameter's is the sum over its broadcast axes; an entry a = -inf has responsibility 0 and
    a row whose logsumexp is -inf has none."""
    B, N, K = a.shape
    event = x.dim() == 2
    shape = (B, K, x.shape[1]) if event else (B, K)
    with torch.enable_grad():                 # (also when called inside an autograd Function's forward)
        x = x.detach().to(dtype)
        a = a.detach().to(dtype).clone().requires_grad_()
        q0 = p0.detach().to(dtype).expand(shape).clone().requires_grad_()
        q1 = None if p1 is None else p1.detach().to(dtype).expand(shape).clone().requires_grad_()
        if event:
            fam = torch_family(family, q0[:, None], None if q1 is None else q1[:, None])
            lp = fam.log_prob(x[:, None, :]).sum(-1)                             # [B, N, K]
        else:
            fam = torch_family(family, q0[:, None, :], None if q1 is None else q1[:, None, :])
            lp = fam.log_prob(x[:, None])                                        # [B, N, K]
        t = a + lp
        lse = torch.logsumexp(t.detach(), -1)                                    # [B, N]
        r = torch.exp(t.detach() - lse[..., None])
        r = torch.where(torch.isneginf(lse)[..., None], torch.zeros_like(r), r)
        # d S / d theta = sum_{n, k} r_nk d t_nk / d theta
        params = [a, q0] + ([q1] if q1 is not None else [])
        grads = torch.autograd.grad((r * t).sum(), params)
    return lse.sum(-1), grads[0], grads[1], (grads[2] if q1 is not None else None)


def row_init(family, N, K, D=None, F=3, G=5, seed=0):
    """float64 CPU tensors a model form is built from: data x [N] or [N, D] drawn from the family's mixture, starting
    component parameters away from the data's, gate features X [N, F] with weights W [F, K] and bias b [K], group
    ids g [N] with weights theta [G, K], and for a third of the rows a known label (the others share the prior pi)."""
    gen = torch.Generator().manual_seed(seed)
    d = 1 if D is None else D
    P0, P1 = family_params(family, K, d, gen)
    x = family_data(family, P0, P1, N, gen)
    P0, P1 = family_params(family, K, d, gen)
    if D is None:
        x, P0, P1 = x[:, 0], P0[:, 0], None if P1 is None else P1[:, 0]
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)           # noqa: E731
    init = {"x": x, "p0": P0, "X": r(N, F), "W": 0.5 * r(F, K), "b": 0.3 * r(K),
            "g": torch.randint(0, G, (N,), generator=gen), "theta": torch.softmax(r(G, K), -1),
            "labeled": torch.rand(N, generator=gen) < 0.3, "label": torch.randint(0, K, (N,), generator=gen),
            "pi": torch.softmax(r(K), -1), "f0": 1.0 + 0.01 * torch.rand(N, generator=gen, dtype=torch.float64),
            "mask": torch.rand(N, generator=gen) > 0.2}
    if P1 is not None:
        init["p1"] = P1
    return init


def make_row_mixture(form, init, dtype, device, family="Normal", backend=None, subsample_size=None):
    """(model, guide, x) over the tensors of ``row_init``: component parameters p0 / p1 of ``family`` as parameters of
    the model, the assignment enumerated under the data plate with per-row probabilities, the observation
    ``Fam(p0[z], p1[z])`` (data [N]) or ``Fam(p0[z], p1[z]).to_event(1)`` (data [N, D]).  ``form``: "experts"
    (``Categorical(logits=X @ W + b)``), "grouped" (``Categorical(theta[g])``), "labels" (known rows one-hot with -inf
    elsewhere, the others a shared prior), "particles" (the gate weights drawn per vectorised particle), "subsample"
    ("experts" on a subsampled plate: pass ``subsample_size``), "detached" ("experts" with the logits detached); and
    with the gate of "experts" the forms the leaf leaves to the generic path: "event" (more features than the
    diagonal leaf takes), "mvn" (a MultivariateNormal observation), "per_row" (p0 varies along the data plate),
    "mask", "value_grad".  ``backend``: the (pyro, distributions, poutine) modules to build on, this package's by
    default."""
    if backend is None:
        import pyro_amd as pyro
        import pyro_amd.distributions as dist
        from pyro_amd import poutine
    else:
        pyro, dist, poutine = backend
    from torch.distributions import constraints

    T = {k: (v.to(device, dtype) if v.is_floating_point() else v.to(device)) for k, v in init.items()}
    x = T["x"]
    if form == "value_grad":
        x = x.clone().requires_grad_()
    N, K = x.shape[0], T["p0"].shape[0]
    event = x.dim() == 2
    c0 = constraints.positive if family in ("Exponential", "Poisson", "Gamma") else constraints.real
    onehot = torch.full((N, K), -float("inf"), dtype=dtype, device=device)
    onehot[torch.arange(N, device=device), T["label"]] = 0.0

    def obs_dist(q0, q1):
        if form == "mvn":
            return dist.MultivariateNormal(q0, scale_tril=torch.diag_embed(q1))
        if family == "Normal":
            d = dist.Normal(q0, q1)
        elif family == "LogNormal":
            d = dist.LogNormal(q0, q1)
        elif family == "Exponential":
            d = dist.Exponential(q0)
        elif family == "Bernoulli":
            d = dist.Bernoulli(logits=q0)
        elif family == "Poisson":
            d = dist.Poisson(q0)
        else:
            d = dist.Gamma(q0, q1)
        return d.to_event(1) if event else d

    def model(x):
        p0 = pyro.param("p0", T["p0"].clone(), constraint=c0)
        p1 = pyro.param("p1", T["p1"].clone(), constraint=constraints.positive) if "p1" in T else None
        if form == "grouped":
            theta = pyro.param("theta", T["theta"].clone(), constraint=constraints.simplex)
        elif form == "labels":
            pi = pyro.param("pi", T["pi"].clone(), constraint=constraints.simplex)
        else:
            if form == "particles":
                W = pyro.sample("W", dist.Normal(torch.zeros_like(T["W"]), 1.0).to_event(2))
            else:
                W = pyro.param("W", T["W"].clone())
            b = pyro.param("b", T["b"].clone())
        with pyro.plate("data", N, subsample_size=subsample_size) as idx:
            rows = (lambda t: t[idx]) if subsample_size is not None else (lambda t: t)    # noqa: E731
            if form == "grouped":
                cat = dist.Categorical(theta[rows(T["g"])])
            elif form == "labels":
                logits = torch.where(rows(T["labeled"])[:, None], rows(onehot), pi.log())
                cat = dist.Categorical(logits=logits)
            else:
                logits = torch.matmul(rows(T["X"]), W) + b
                if logits.dim() > 2:             # (a draw of W per particle: [P, 1, N, K])
                    logits = logits.squeeze(-3)
                cat = dist.Categorical(logits=logits.detach() if form == "detached" else logits)
            z = pyro.sample("z", cat, infer={"enumerate": "parallel"})
            q0 = p0[z]
            if form == "per_row":
                f0 = rows(T["f0"])
                q0 = q0 * (f0[:, None] if event else f0)
            q1 = None if p1 is None else p1[z]
            if form == "mask":
                with poutine.mask(mask=rows(T["mask"])):
                    pyro.sample("x", obs_dist(q0, q1), obs=rows(x))
            else:
                pyro.sample("x", obs_dist(q0, q1), obs=rows(x))

    def guide(x):
        if form == "particles":
            qW = pyro.param("qW", T["W"].clone())
            pyro.sample("W", dist.Normal(qW, 0.1).to_event(2))

    return model, guide, x


def flat_params(p, B, K):
    """p [B | 1, K | 1] -> (flat contiguous tensor addressed b * bs + k * s, s, bs): the scalar leaf's convention."""
    if p is None:
        return None, 0, 0
    Bp, Kp = p.shape
    return p.contiguous().reshape(-1), (1 if Kp == K and K > 1 else 0), (Kp if Bp == B and B > 1 else 0)


def unflat_params(p, s, bs, B, K):
    """the [B, K] view of a flat parameter addressed b * bs + k * s (stride 0: shared)"""
    return None if p is None else p.as_strided((B, K), (bs, s))
