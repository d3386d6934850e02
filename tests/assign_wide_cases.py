"""Shared pieces of the tests of the wide leaves' assignment kernels (csrc/mixture_assign_wide.hip): the committed
kernel cases (float64 CPU inputs from a seed), their float64 torch scores, float64 stand-ins for
kernels.mixture_assign_event / mixture_assign_mvn, and a fitted-style full-covariance mixture whose scale_tril is a
true lower triangle.  What decides (map_reference, draw_reference, philox_uniforms) is tests/assign_cases.py's."""
import torch

from tests.assign_cases import assign_scores, draw_reference, map_reference, philox_uniforms
from tests.event_mixture_cases import FAMILIES, dist_id, family_data, family_params
from tests.mvn_mixture_cases import gmm_data, random_tril

# (family, D, K, N, B, share): a sparse cross of D in {1, 9, 63, 65, 300, 1024} (one feature chunk, ragged, several,
# the limit), K in {1, 3, 16, 17, 64} (one chunk of 16 components, ragged, a second chunk, the limit), N in {1, 255,
# 257, 1031} (against the 256-row tile), B in {1, 3}; parameters shared over k ("k": p1 -- p0 for one-parameter
# families), over d ("d": every parameter) and over b ("b") in turn
EVENT_CASES = (
    ("Bernoulli", 1, 1, 1, 1, None),
    ("Normal", 9, 3, 255, 3, "k"),
    ("LogNormal", 63, 16, 257, 1, "d"),
    ("Exponential", 65, 17, 1031, 3, "b"),
    ("Poisson", 300, 64, 257, 1, None),
    ("Gamma", 1024, 3, 255, 3, None),
    ("Bernoulli", 1024, 16, 1031, 1, None),
    ("Gamma", 9, 64, 1, 3, "k"),
    ("Normal", 300, 17, 1031, 1, "d"),
)

# (D, K, N, B, share): D in {1, 3, 8, 9, 17, 33, 64} (every padded D of 8, 16, 32, 64 and a ragged D inside each),
# K in {1, 5, 64} and 20 (the kernel's score storage of 16, 32 and 64), the same N and B; "k": W one matrix for every
# component, "loc_k": loc one vector for every component, "b": both one set for every b
MVN_CASES = (
    (1, 1, 1, 1, None),
    (3, 5, 255, 3, "k"),
    (8, 64, 257, 1, None),
    (9, 5, 1031, 3, "b"),
    (17, 5, 257, 1, "loc_k"),
    (33, 64, 255, 1, None),
    (64, 5, 1031, 3, None),
    (8, 20, 255, 1, None),
)


def event_case(family, D, K, N, B, share, seed=0):
    """float64 CPU inputs: x [N, D] drawn from the family's mixture, a [B, K] log-weights, p0 / p1 [B | 1, K | 1,
    D | 1] (p1 None for one-parameter families)."""
    g = torch.Generator().manual_seed(1000 + seed)
    P0, P1 = family_params(family, K, D, g)
    x = family_data(family, P0, P1, N, g)
    ps = [family_params(family, K, D, g) for _ in range(1 if share == "b" else B)]
    p0 = torch.stack([q[0] for q in ps])
    p1 = None if P1 is None else torch.stack([q[1] for q in ps])
    if share == "k":
        if p1 is None:
            p0 = p0[:, :1]
        else:
            p1 = p1[:, :1]
    if share == "d":
        p0, p1 = p0[..., :1], None if p1 is None else p1[..., :1]
    a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    return {"x": x, "a": a, "p0": p0.contiguous(), "p1": None if p1 is None else p1.contiguous()}


def mvn_case(D, K, N, B, share, seed=0, shift=0.0):
    """float64 CPU inputs: x [N, D] around K centres, a [B, K], loc [B | 1, K | 1, D], L [B | 1, K | 1, D, D] lower
    triangular (tests/mvn_mixture_cases.py's data and factors).  ``shift``: added to the data and to every loc -- with
    1e4 the badly scaled case |x| >> the spread."""
    g = torch.Generator().manual_seed(2000 + seed)
    x, centres = gmm_data(N, K, D, g)
    Bp = 1 if share == "b" else B
    loc = torch.stack([centres + 0.3 * torch.randn(K, D, generator=g, dtype=torch.float64) for _ in range(Bp)])
    L = torch.stack([random_tril(K, D, g, spread=0.5) * 1.5 for _ in range(Bp)])
    if share == "k":
        L = L[:, :1]
    if share == "loc_k":
        loc = loc[:, :1]
    a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    return {"x": x + shift, "a": a, "loc": (loc + shift).contiguous(), "L": L.contiguous()}


def diffuse_case(N=1031, K=5, B=3, D=9):
    """float64 CPU inputs whose components overlap (locations 0.3 apart against a spread of 1), so that a row's
    posterior is spread over the components and its draw depends on the uniform: (x, a, loc, scale) for the event
    kernel's Normal and (x, a, loc, W) for the full-covariance kernel, W a well-conditioned lower triangle."""
    g = torch.Generator().manual_seed(3000)
    x = torch.randn(N, D, generator=g, dtype=torch.float64)
    loc = 0.3 * torch.randn(B, K, D, generator=g, dtype=torch.float64)
    a = torch.log_softmax(torch.randn(B, K, generator=g, dtype=torch.float64), -1)
    W = inverse_tril(torch.stack([random_tril(K, D, g, spread=0.3) + 0.5 * torch.eye(D, dtype=torch.float64)
                                  for _ in range(B)])).contiguous()
    return (x, a, loc, torch.ones_like(loc)), (x, a, loc, W)


def inverse_tril(L):
    """W = L^-1 in float64 (lower triangular), as the package forms it for the leaves"""
    eye = torch.eye(L.shape[-1], dtype=torch.float64, device=L.device)
    return torch.linalg.solve_triangular(L.to(torch.float64), eye, upper=False)


def mvn_scores(x, a, loc, W):
    """t [B, N, K] in float64: a[b, k] + log MultivariateNormal(x[n] | loc[b, k], scale_tril = W[b, k]^-1) by torch's
    own log_prob.  x [N, D]; a [B, K]; loc [B | 1, K | 1, D]; W [B | 1, K | 1, D, D]."""
    dt = torch.float64
    L = inverse_tril(torch.tril(W.detach().to(dt)))
    mvn = torch.distributions.MultivariateNormal(loc.detach().to(dt)[:, None], scale_tril=L[:, None],
                                                 validate_args=False)
    return a.detach().to(dt)[:, None, :] + mvn.log_prob(x.detach().to(dt)[:, None, :])


def pick(t, mode, dtype, seed, offset):
    if mode == 0:
        return map_reference(t, 0.0)[0]
    B, N = t.shape[:2]
    return draw_reference(t, philox_uniforms(B, N, dtype, seed, offset, t.device), 0.0)[0]


def wide_standins(calls):
    """float64 torch stand-ins for kernels.mixture_assign_event / mixture_assign_mvn that note every call in ``calls``
    as ("event", family id, x's shape, a's shape, p0's shape, p1's shape or None, mode) or ("mvn", x's shape, a's
    shape, loc's shape, W's shape, mode)."""
    names = {dist_id(f): f for f in FAMILIES}

    def event(dist, x, a, p0, p1, mode=0, seed=0, offset=0, offset_dev=None):
        calls.append(("event", int(dist), tuple(x.shape), tuple(a.shape), tuple(p0.shape),
                      None if p1 is None else tuple(p1.shape), int(mode)))
        assert x.dim() == 2 and a.dim() == 2 and p0.dim() == 3 and (p1 is None or p1.dim() == 3)
        assert x.is_contiguous() and a.is_contiguous() and p0.is_contiguous() and (p1 is None or p1.is_contiguous())
        assert not (x.requires_grad or a.requires_grad or p0.requires_grad)
        return pick(assign_scores(names[int(dist)], x, a, p0, p1), mode, x.dtype, seed, offset)

    def mvn(x, a, loc, W, mode=0, seed=0, offset=0, offset_dev=None):
        calls.append(("mvn", tuple(x.shape), tuple(a.shape), tuple(loc.shape), tuple(W.shape), int(mode)))
        assert x.dim() == 2 and a.dim() == 2 and loc.dim() == 3 and W.dim() == 4
        assert x.is_contiguous() and a.is_contiguous() and loc.is_contiguous() and W.is_contiguous()
        assert not (x.requires_grad or a.requires_grad or loc.requires_grad or W.requires_grad)
        return pick(mvn_scores(x, a, loc, W), mode, x.dtype, seed, offset)

    return event, mvn


def fitted_mvn_mixture(form, device, dtype, N, K, B=3, D=3):
    """A fitted-style mixture with fixed parameters and the observation ``MultivariateNormal(locs[z],
    scale_tril=L[z])`` with a true lower-triangular L, whose model returns z: ``form`` "plain" (weights shared by the
    rows), "sets" (B vectorised parameter sets under an outer plate at dim -2) or "gate" (per-row weights)."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist

    g = torch.Generator().manual_seed(29)
    x, centres = gmm_data(N, K, D, g)
    locs = torch.stack([centres + 0.3 * torch.randn(K, D, generator=g, dtype=torch.float64) for _ in range(B)])
    Ls = torch.stack([random_tril(K, D, g, spread=0.5) * 1.5 for _ in range(B)])
    x, locs, Ls = x.to(device, dtype), locs.to(device, dtype), Ls.to(device, dtype)
    pi = torch.softmax(torch.randn(K, generator=g, dtype=torch.float64), -1).to(device, dtype)
    X = torch.randn(N, 3, generator=g, dtype=torch.float64).to(device, dtype)
    Wg = (0.5 * torch.randn(3, K, generator=g, dtype=torch.float64)).to(device, dtype)
    rows_b = torch.arange(B, device=device)[:, None]

    def model():
        if form == "sets":
            with pyro.plate("sets", B, dim=-2), pyro.plate("data", N, dim=-1):
                z = pyro.sample("z", dist.Categorical(pi), infer={"enumerate": "parallel"})
                pyro.sample("obs", dist.MultivariateNormal(locs[rows_b, z], scale_tril=Ls[rows_b, z]), obs=x)
            return z
        with pyro.plate("data", N, dim=-1):
            cat = dist.Categorical(logits=X @ Wg) if form == "gate" else dist.Categorical(pi)
            z = pyro.sample("z", cat, infer={"enumerate": "parallel"})
            pyro.sample("obs", dist.MultivariateNormal(locs[0][z], scale_tril=Ls[0][z]), obs=x)
        return z

    return model
