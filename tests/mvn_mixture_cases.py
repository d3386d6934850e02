"""Shared pieces of the full-covariance MultivariateNormal mixture tests: a float64 torch statement of what
pa_mixture_mvn_fwd_bwd returns, and the enumerated Gaussian mixture model in its accepted and rejected forms."""
import math

import torch


def mvn_leaf_reference(x, a, loc, W):
    """float64 torch: (S [B], R [B, K], m [B, K, D], G [B, K, D, D]) of kernels.mixture_mvn_fwd_bwd -- the same
    arguments (x [N, D]; a [B, K]; loc [B | 1, K | 1, D]; W [B | 1, K | 1, D, D] lower triangular)."""
    x = x.detach().double()
    B, K = a.shape
    N, D = x.shape
    Wd = torch.tril(W.detach().double()).expand(B, K, D, D)
    d = x[None, None] - loc.detach().double().expand(B, K, D)[:, :, None, :]              # [B, K, N, D]
    z = torch.einsum("bkij,bknj->bkni", Wd, d)
    logdet = torch.log(torch.diagonal(Wd, dim1=-2, dim2=-1)).sum(-1)                         # [B, K]
    t = (a.detach().double() + logdet)[:, :, None] - 0.5 * D * math.log(2 * math.pi) - 0.5 * (z * z).sum(-1)
    lse = torch.logsumexp(t, 1)                                                              # [B, N]
    r = torch.exp(t - lse[:, None])
    r = torch.where(torch.isneginf(lse)[:, None], torch.zeros_like(r), r)
    R = r.sum(-1)
    m = torch.einsum("bkn,bkni->bki", r, z)
    G = torch.tril(torch.einsum("bkn,bkni,bknj->bkij", r, z, d))
    return lse.sum(-1), R, m, G


def random_tril(K, D, gen, spread=0.3):
    """[K, D, D] lower-triangular scale factors with a positive diagonal, well conditioned."""
    L = torch.randn(K, D, D, generator=gen, dtype=torch.float64) * spread / math.sqrt(D)
    L = torch.tril(L, -1) + torch.diag_embed(0.5 + torch.rand(K, D, generator=gen, dtype=torch.float64))
    return L


def gmm_data(N, K, D, gen):
    centres = 4.0 * torch.randn(K, D, generator=gen, dtype=torch.float64)
    z = torch.randint(0, K, (N,), generator=gen)
    return centres[z] + torch.randn(N, D, generator=gen, dtype=torch.float64), centres


def make_gmm(N, K, D, dtype, device, form="tril", subsample_size=None, seed=0):
    """(model, guide, x): Dirichlet weights (a Delta guide), per-component ``locs`` and a full-covariance factor as
    parameters of the guide-free model part, the assignment enumerated under the data plate.  ``form``: how the
    observation is written -- "tril" (scale_tril=L[z]; "particles": the same under vectorised
    particles), "tril_shared" (one scale_tril for every component), "cov" (covariance_matrix=), "prec" (precision_matrix=), "loc_shared" (loc shared, L[z]), and the forms the leaf must
    leave to the generic path: "mask", "loc_per_row", "row_weights", "value_grad"."""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from torch.distributions import constraints

    gen = torch.Generator().manual_seed(seed)
    x, centres = gmm_data(N, K, D, gen)
    x = x.to(device, dtype)
    locs0 = (centres + 0.3 * torch.randn(K, D, generator=gen, dtype=torch.float64)).to(device, dtype)
    L0 = random_tril(K, D, gen, spread=0.5).to(device, dtype) * 1.5
    if form == "loc_per_row":
        shift0 = (0.01 * torch.randn(N, D, generator=gen, dtype=torch.float64)).to(device, dtype)
    if form == "row_weights":
        rw0 = torch.rand(N, K, generator=gen, dtype=torch.float64).to(device, dtype) + 0.5
    if form == "mask":
        mask0 = torch.rand(N, generator=gen) > 0.2
    if form == "value_grad":
        x = x.clone().requires_grad_()

    def model(x):
        w = pyro.sample("w", dist.Dirichlet(torch.ones(K, dtype=dtype, device=device)))
        locs = pyro.param("locs", locs0.clone())
        if form == "tril_shared":
            scale = pyro.param("scale_tril", L0[0].clone(), constraint=constraints.lower_cholesky)
        else:
            scale = pyro.param("scale_tril", L0.clone(), constraint=constraints.lower_cholesky)
        with pyro.plate("data", N, subsample_size=subsample_size) as idx:
            xs = x[idx] if subsample_size is not None else x
            probs = w
            if form == "row_weights":
                rw = pyro.param("row_weights", rw0.clone(), constraint=constraints.positive)
                probs = w * (rw[idx] if subsample_size is not None else rw)
            z = pyro.sample("z", dist.Categorical(probs), infer={"enumerate": "parallel"})
            loc = locs[z]
            if form == "loc_shared":
                loc = locs[0]
            elif form == "loc_per_row":
                shift = pyro.param("shift", shift0.clone())
                loc = loc + (shift[idx] if subsample_size is not None else shift)
            Lz = scale if form == "tril_shared" else scale[z]
            if form == "cov":
                d = dist.MultivariateNormal(loc, covariance_matrix=Lz @ Lz.transpose(-1, -2))
            elif form == "prec":
                d = dist.MultivariateNormal(loc, precision_matrix=torch.cholesky_inverse(Lz))
            else:
                d = dist.MultivariateNormal(loc, scale_tril=Lz)
            if form == "mask":
                with poutine.mask(mask=mask0.to(device)):
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
