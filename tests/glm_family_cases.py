"""Cases of the fused plated regression sites (csrc/glm_family.hip, distributions/families.py::_LinearPredictor):
the model text of the four sites, a torch restatement of what they compute (any dtype: float64 is the reference of
the device tests, float32 the project's four-times yardstick), the magnitudes the float32 floor scales with, and the
kernel-level case tables.  tests/test_glm_family_host.py checks the restatement against tests/golden/glm_families.npz
(written by the unmodified reference); the device tests lean on it."""
import math
import os

import numpy as np
import torch

FAMILIES = ("normal", "student_t", "poisson", "binomial")
FAMILY_ID = {"normal": 0, "student_t": 1, "poisson": 2, "binomial": 3}       # PA_GLM_* of include/pyro_amd.h
AUX_NAMES = {"normal": ("sigma",), "student_t": ("nu", "sigma"), "poisson": (), "binomial": ()}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glm_families.npz")
# fixture models: the four families, Binomial once with a per-row count and once with a scalar one
GOLDEN_MODELS = ("normal", "student_t", "poisson", "binomial_rows", "binomial_scalar")
SCALAR_COUNT = 12.0
F32_FLOOR = 4.0 * 2.0 ** -23


def family_of(model_name):
    return model_name.split("_rows")[0].split("_scalar")[0]


# ---- the model text (run by the reference to make the fixture, and by the package in the tests) ---------------
def make_model(pyro, dist, poutine, name):
    """``name`` of GOLDEN_MODELS -> model(X, y, mask, plate_size, count=None).  Latents carry flat (masked-out)
    priors so that the step's loss is the observed site alone."""
    family = family_of(name)

    def model(X, y, mask, plate_size, count=None):
        N, D = X.shape
        zero, one = X.new_zeros(()), X.new_ones(())
        w = pyro.sample("w", dist.Normal(X.new_zeros(D), one).to_event(1).mask(False))
        b = pyro.sample("b", dist.Normal(zero, one).mask(False))
        if family in ("normal", "student_t"):
            sigma = pyro.sample("sigma", dist.LogNormal(zero, one).mask(False))
        if family == "student_t":
            nu = pyro.sample("nu", dist.Gamma(2.0 * one, 0.1 * one).mask(False))
        with pyro.plate("data", plate_size, subsample_size=N), poutine.mask(mask=mask):
            eta = w @ X.t()
            if eta.dim() > 1:
                eta = eta.squeeze(-2)
            eta = eta + b
            if family == "normal":
                pyro.sample("obs", dist.Normal(eta, sigma), obs=y)
            elif family == "student_t":
                pyro.sample("obs", dist.StudentT(nu, eta, sigma), obs=y)
            elif family == "poisson":
                pyro.sample("obs", dist.Poisson(torch.exp(eta)), obs=y)
            else:
                pyro.sample("obs", dist.Binomial(count, logits=eta), obs=y)
    return model


# ---- torch restatement ------------------------------------------------------------------------------------------
def _softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def site_terms(family, eta, y, aux, count, full):
    """Signed addends of the log density of every (particle, row): a list of [P, N] tensors.  eta [P, N], y [N],
    aux: tuple of [P, 1] tensors, count: [N] tensor / number / None.  ``full``: with the normaliser that depends on
    the particle only (what the site class returns); without it, what the kernel returns."""
    P, N = eta.shape
    ones = torch.ones_like(eta)
    if family == "normal":
        sigma, = aux
        z = (y - eta) / sigma
        out = [-0.5 * z * z]
        if full:
            out += [-sigma.log() * ones, -0.5 * math.log(2.0 * math.pi) * ones]
    elif family == "student_t":
        nu, sigma = aux
        z = (y - eta) / sigma
        out = [-0.5 * (nu + 1.0) * torch.log1p(z * z / nu)]
        if full:
            out += [torch.lgamma(0.5 * (nu + 1.0)) * ones, -torch.lgamma(0.5 * nu) * ones,
                    -0.5 * (nu * math.pi).log() * ones, -sigma.log() * ones]
    elif family == "poisson":
        out = [y * eta, -torch.exp(eta), -torch.lgamma(y + 1.0) * ones]
    else:
        n = count if isinstance(count, torch.Tensor) else torch.full_like(y, float(count))
        out = [y * eta, -n * _softplus(eta), torch.lgamma(n + 1.0) * ones, -torch.lgamma(y + 1.0) * ones,
               -torch.lgamma(n - y + 1.0) * ones]
    return out


def torch_route(*args):
    with torch.enable_grad():
        return _torch_route(*args)


def _torch_route(family, X, y, w, b, aux, count, mask, scale, dtype, full):
    """The site written with torch operators in ``dtype`` on the CPU, gradients by autograd:
    {"s" [P], "gw" [P, D], "gb" [P] or None, "gaux" [P, A] or None}.  X [N, D], w [P, D], b [P] or None,
    aux [P, A] or None."""
    c = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)      # noqa: E731
    X, y, w, b, aux = c(X), c(y), c(w), c(b), c(aux)
    if isinstance(count, torch.Tensor):
        count = c(count)
    w = w.clone().requires_grad_(True)
    leaves = [w]
    if b is not None:
        b = b.clone().requires_grad_(True)
        leaves.append(b)
    if aux is not None and aux.shape[1] > 0:
        aux = aux.clone().requires_grad_(True)
        leaves.append(aux)
        cols = tuple(aux[:, k:k + 1] for k in range(aux.shape[1]))
    else:
        aux, cols = None, ()
    eta = w @ X.t()
    if b is not None:
        eta = eta + b[:, None]
    lp = sum(site_terms(family, eta, y, cols, count, full))
    if mask is not None:
        lp = torch.where(torch.as_tensor(mask).cpu().bool(), lp, torch.zeros_like(lp))
    s = lp.sum(-1) * scale
    grads = torch.autograd.grad(s.sum(), leaves)
    out = {"s": s.detach(), "gw": grads[0], "gb": None, "gaux": None}
    k = 1
    if b is not None:
        out["gb"] = grads[k]
        k += 1
    if aux is not None:
        out["gaux"] = grads[k]
    return out


def magnitudes(family, X, y, w, b, aux, count, mask, scale, full):
    """Per output entry, the float64 sum of the absolute values of the addends that make it up (the magnitude a
    float32 sum's rounding scales with): same keys and shapes as torch_route."""
    c = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().to(torch.float64)     # noqa: E731
    X, y, w, b, aux = c(X), c(y), c(w), c(b), c(aux)
    if isinstance(count, torch.Tensor):
        count = c(count)
    P, N = w.shape[0], X.shape[0]
    eta = w @ X.t() + (0.0 if b is None else b[:, None])
    m = torch.ones(N, dtype=torch.float64) if mask is None else torch.as_tensor(mask).cpu().to(torch.float64)
    cols = () if aux is None else tuple(aux[:, k:k + 1] for k in range(aux.shape[1]))
    A = {"s": sum(t.abs() for t in site_terms(family, eta, y, cols, count, full)) @ m * scale}
    # addends of d/d eta and d/d aux per (particle, row)
    if family == "normal":
        sigma, = cols
        z = (y - eta) / sigma
        deta = [z / sigma]
        daux = [[z * z / sigma] + ([1.0 / sigma * torch.ones_like(eta)] if full else [])]
    elif family == "student_t":
        nu, sigma = cols
        z = (y - eta) / sigma
        q = z * z / (nu + z * z)
        deta = [(nu + 1.0) * z / ((nu + z * z) * sigma)]
        dnu = [0.5 * torch.log1p(z * z / nu), (nu + 1.0) * q / (2.0 * nu)]
        dsig = [(nu + 1.0) * q / sigma]
        if full:
            one = torch.ones_like(eta)
            dnu += [0.5 * torch.digamma(0.5 * (nu + 1.0)) * one, 0.5 * torch.digamma(0.5 * nu) * one,
                    0.5 / nu * one]
            dsig += [1.0 / sigma * one]
        daux = [dnu, dsig]
    elif family == "poisson":
        deta, daux = [y * torch.ones_like(eta), torch.exp(eta)], []
    else:
        n = count if isinstance(count, torch.Tensor) else torch.full_like(y, float(count))
        deta, daux = [y * torch.ones_like(eta), n * torch.sigmoid(eta)], []
    g = sum(t.abs() for t in deta) * m
    A["gw"] = g @ X.abs() * scale
    A["gb"] = None if b is None else g.sum(-1) * scale
    A["gaux"] = None if not daux else torch.stack([sum(t.abs() for t in col) @ m for col in daux], dim=-1) * scale
    return A


def bounds(family, X, y, w, b, aux, count, mask, scale, full):
    """(reference, bound) per output: the float64 torch route, and per entry max(4 * e32, 4 * 2^-23 * A) with e32
    the error of the float32 torch route on the CPU against it."""
    ref = torch_route(family, X, y, w, b, aux, count, mask, scale, torch.float64, full)
    f32 = torch_route(family, X, y, w, b, aux, count, mask, scale, torch.float32, full)
    A = magnitudes(family, X, y, w, b, aux, count, mask, scale, full)
    bound = {}
    for k, r in ref.items():
        if r is None:
            bound[k] = None
            continue
        e32 = (f32[k].to(torch.float64) - r).abs()
        bound[k] = torch.maximum(4.0 * e32, F32_FLOOR * A[k])
    return ref, bound


# ---- inputs -------------------------------------------------------------------------------------------------------
def make_inputs(family, N, D, P, bias, masked, seed, per_row_count=True):
    """X standard normal, w scaled so that |eta| <= 6, sigma in [0.3, 3], nu in [1.5, 30], counts in 1..20 with
    y <= n, Poisson y drawn at the model's own rates (float32 arrays, numpy generator)."""
    g = np.random.default_rng(seed)
    X = g.standard_normal((N, D)).astype(np.float32)
    w = g.standard_normal((P, D)).astype(np.float32)
    b = (0.5 * g.standard_normal(P)).astype(np.float32) if bias else None
    eta = w.astype(np.float64) @ X.astype(np.float64).T + (0.0 if b is None else b[:, None].astype(np.float64))
    top = np.abs(eta).max() if N else 0.0
    if top > 6.0:
        w = (w * np.float32(5.9 / top)).astype(np.float32)
        if b is not None:
            b = (b * np.float32(5.9 / top)).astype(np.float32)
        eta = w.astype(np.float64) @ X.astype(np.float64).T + (0.0 if b is None else b[:, None].astype(np.float64))
    aux, count = None, None
    row = eta[g.integers(0, P)] if N else np.zeros(0)
    if family == "normal":
        aux = g.uniform(0.3, 3.0, (P, 1)).astype(np.float32)
        y = row + g.standard_normal(N)
    elif family == "student_t":
        aux = np.stack([g.uniform(1.5, 30.0, P), g.uniform(0.3, 3.0, P)], axis=1).astype(np.float32)
        y = row + g.standard_t(3.0, N)
    elif family == "poisson":
        y = g.poisson(np.exp(row)).astype(np.float64)
    else:
        n = g.integers(1, 21, N)
        if not per_row_count:
            n = np.full(N, int(SCALAR_COUNT))
        y = g.binomial(n, 1.0 / (1.0 + np.exp(-row))).astype(np.float64)
        count = torch.as_tensor(n.astype(np.float32)) if per_row_count else SCALAR_COUNT
    mask = torch.as_tensor(g.random(N) > 0.2) if masked else None
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float32))     # noqa: E731
    return {"X": t(X), "y": t(y), "w": t(w), "b": t(b), "aux": t(aux), "count": count, "mask": mask}


# ---- kernel-level case table: (N, D, P, bias, masked, scale, max_blocks) --------------------------------------------
# Every N of {1, 31, 32, 33, 127, 128, 129, 300}, 300 on one workgroup and 1100 on two (several trips of the tile
# loop, the last one ragged); every D of {1, 3, 4, 31, 32, 33, 64, 127, 128} (scalar and float4 staging; one, two and
# four feature tiles); every P of {1, 31, 32, 33, 64, 65} (one and two particle tiles, one to three passes); each
# with and without bias and mask, scale 1 and 3.5.  Not the cross product: each value of one axis meets a spread of
# the others.
def kernel_cases():
    Ns = (1, 31, 32, 33, 127, 128, 129, 300)
    Ds = (1, 3, 4, 31, 32, 33, 64, 127, 128)
    Ps = (1, 31, 32, 33, 64, 65)
    cases = []
    k = 0
    for i, N in enumerate(Ns):                       # every N, D and P walking along
        for j in range(2):
            D, P = Ds[(2 * i + j) % len(Ds)], Ps[(i + 3 * j) % len(Ps)]
            cases.append((N, D, P, k % 2 == 0, k % 3 != 0, 1.0 if k % 4 < 2 else 3.5, 0))
            k += 1
    for i, D in enumerate(Ds):                       # every D at a multi-tile N
        cases.append((129 if i % 2 else 300, D, Ps[(i + 1) % len(Ps)], i % 2 == 1, i % 3 == 0,
                      3.5 if i % 2 else 1.0, 0))
    for i, P in enumerate(Ps):                       # every P at both staging forms
        cases.append((127, 32 if i % 2 else 5, P, i % 2 == 0, i % 2 == 1, 1.0 if i % 2 else 3.5, 0))
        cases.append((33, 4 if i % 2 else 33, P, i % 2 == 1, i % 2 == 0, 3.5, 0))
    for D, P in ((32, 64), (5, 33), (64, 3), (128, 32)):    # several trips per wave, the last one ragged
        cases.append((300, D, P, True, True, 3.5, 1))
        cases.append((1100, D, P, D != 5, D == 5, 1.0, 2))
    return cases


def case_id(c):
    return "N%d-D%d-P%d-%s-%s-s%g-mb%d" % (c[0], c[1], c[2], "b" if c[3] else "nob", "m" if c[4] else "nom", c[5],
                                            c[6])


def make_guide(pyro, dist, latents):
    """Point-mass guide at ``latents`` (name -> tensor carrying the particle dims), each a parameter ``<name>_q``:
    with the model's flat priors the step's loss is -(1 / P) * sum_p ll_p and the parameters' gradients are the
    observed site's."""
    def guide(X, y, mask, plate_size, count=None):
        for k, v in latents.items():
            p = pyro.param(k + "_q", v.detach().clone())
            pyro.sample(k, dist.Delta(p, event_dim=1 if k == "w" else 0))
    return guide


def assert_within(got, ref, bound, what):
    """Entry by entry: |got - ref| <= bound (float64 on the CPU); non-finite entries fail."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64).reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %d of %d entries out of bound; first: entry %d got %r want %r error %.3e bound %.3e"
                             % (what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]),
                                float(ref.reshape(-1)[i]), float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])))


def assert_step_within(loss, grads, ref, bound, family, P):
    """One Trace_ELBO step of make_model / make_guide against ``bounds(..., full=True)``: loss = -(1 / P) sum_p ll_p
    (its bound: the sum of the particles' bounds), the parameters' gradients -(1 / P) times the site's."""
    assert_within(torch.as_tensor(float(loss)), -ref["s"].sum() / P, bound["s"].sum() / P, "loss")
    assert_within(grads["w_q"], -ref["gw"] / P, bound["gw"] / P, "grad w")
    assert_within(grads["b_q"], -ref["gb"] / P, bound["gb"] / P, "grad b")
    for k, a in enumerate(AUX_NAMES[family]):
        assert_within(grads[a + "_q"], -ref["gaux"][:, k] / P, bound["gaux"][:, k] / P, "grad " + a)
