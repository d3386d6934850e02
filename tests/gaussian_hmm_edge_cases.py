"""The edge cases of the GaussianHMM kernels that tests/test_gaussian_hmm_edges_host.py and _gpu.py share: the case
generators (seeded numpy, float64, made once, read-only), the leaves-to-kernel-layout graph, the torch route on the
CPU as the target, and the error kinds.  The input recipe is the one of tests/golden/make_golden_gaussian_hmm.py: F at
spectral norm 0.9, H = randn / sqrt(hidden), covariances A A^T / n + 0.5 I, locations 0.3 randn, x = 2 randn.

A case is named by a key (a tuple):

    ("A", layout, h, o)              the layout matrix, B = 3, T = 5 (LAYOUTS; fixtures at the narrow width (3, 2) in
                                     tests/golden/gaussian_hmm_edges.npz, made by make_golden_gaussian_hmm_edges.py)
    ("B", h, o, T, per_step)         the width border and the shortest chains, B = 2, per-series
    ("D", recipe, h, o, seed)        ill-conditioned inputs, B = 2, T = 20, per-series time-homogeneous (RECIPES)

Every leaf carries both leading axes explicitly: a timed leaf is [B | 1, T | 1, ...], m0 and L0 are [B | 1, ...] -- the
layouts of kernels.gaussian_hmm_fwd_bwd, so ``parts`` is the whole graph between the leaves and the kernel.
"""
import functools
import os
import zlib

import numpy as np
import torch

import pyro_amd.distributions as dist
from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc

NAMES = gc.NAMES
TIMED = ("F", "q", "Lq", "H", "r", "Lr")
CPU = torch.device("cpu")
F32, F64 = torch.float32, torch.float64
FLOOR32 = 4 * 2.0 ** -23          # four float32 roundings (tests/gaussian_hmm_prior_cases.py)
SEEDED = 3                        # seeded draws per case
A_B, A_T = 3, 5
A_WIDTHS = ((3, 2), (9, 2))
KINDS = ("log_prob", "grad", "filter", "maps", "draws", "prior_x", "prior_z")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_hmm_edges.npz")


def _layouts():
    """name -> (per-series? x 6, per-step? x 6 in the order of TIMED, m0 and P0 shared?)"""
    yes, no = (True,) * 6, (False,) * 6
    out = {}
    for k, name in enumerate(TIMED):
        one = tuple(i == k for i in range(6))
        rest = tuple(i != k for i in range(6))
        out["step_" + name] = (yes, one, False)            # only parameter k is per-step
        out["hom_" + name] = (yes, rest, False)            # only parameter k is time-homogeneous
        out["shared_" + name] = (rest, yes, False)         # only parameter k is shared across the series
        out["series_" + name] = (one, no, True)            # only parameter k is per-series; m0, P0 shared as [1, ...]
    rng = np.random.default_rng(20241019)
    for i in range(2):                                     # batch sharing and time layout drawn independently
        per_series = tuple(bool(v) for v in rng.integers(0, 2, 6))
        per_step = tuple(bool(v) for v in rng.integers(0, 2, 6))
        assert any(per_series) and not all(per_series) and any(per_step) and not all(per_step)
        out["mix%d" % i] = (per_series, per_step, bool(i))
    return out


LAYOUTS = _layouts()
A_KEYS = tuple(("A", lay, h, o) for h, o in A_WIDTHS for lay in LAYOUTS)
B_SHAPES = ((8, 8), (7, 8), (9, 1), (1, 9), (8, 9), (9, 8), (16, 1), (1, 16), (15, 16), (16, 15), (1, 2), (2, 1))
B_TS = (1, 2, 3)
B_PER_STEP = ((9, 8), (16, 15))                            # at T = 2 and 3: a per-step variant as well
RECIPES = ("noiseless", "shifted", "diffuse")
D_SCALES = {"noiseless": 1e-2, "shifted": 1e3, "diffuse": 1e2}       # Lr x 1e-2 (R ~ 1e-4); r and x + 1e3; L0 x 1e2
D_SHAPES = ((4, 4), (9, 2), (16, 16))
D_SEEDS = tuple(range(100, 108))
D_B, D_T = 2, 20


def d_keys(recipe, shape):
    """the eight seeds' keys of a recipe x shape"""
    return [("D", recipe) + shape + (seed,) for seed in D_SEEDS]


def make_inputs(rng, B, T, h, o, per_series, per_step, init_shared=False):
    """{name: float64 array} of NAMES for the layout (see _layouts)"""
    def lead(name):
        i = TIMED.index(name)
        return (B if per_series[i] else 1, T if per_step[i] else 1)

    def randn(*shape):
        return rng.standard_normal(shape)

    def tril(shape, n):
        A = randn(*(shape + (n, n)))
        return np.linalg.cholesky(A @ np.swapaxes(A, -1, -2) / n + 0.5 * np.eye(n))

    B0 = 1 if init_shared else B
    F = randn(*(lead("F") + (h, h)))
    F = F * (0.9 / np.linalg.norm(F, ord=2, axis=(-2, -1)))[..., None, None]
    return {"m0": 0.3 * randn(B0, h), "L0": tril((B0,), h), "F": F, "q": 0.3 * randn(*(lead("q") + (h,))),
            "Lq": tril(lead("Lq"), h), "H": randn(*(lead("H") + (h, o))) / np.sqrt(h),
            "r": 0.3 * randn(*(lead("r") + (o,))), "Lr": tril(lead("Lr"), o), "x": 2.0 * randn(B, T, o)}


@functools.lru_cache(maxsize=None)
def inputs(key):
    """{name: read-only float64 array} of the case"""
    yes, no = (True,) * 6, (False,) * 6
    if key[0] == "A":
        _, lay, h, o = key
        rng = np.random.default_rng([20241019, list(LAYOUTS).index(lay), h, o])
        out = make_inputs(rng, A_B, A_T, h, o, *LAYOUTS[lay])
    elif key[0] == "B":
        _, h, o, T, het = key
        out = make_inputs(np.random.default_rng([20241020, h, o, T, int(het)]), 2, T, h, o, yes, yes if het else no)
    else:
        _, recipe, h, o, seed = key
        out = make_inputs(np.random.default_rng(seed), D_B, D_T, h, o, yes, no)
        name, _, scale = recipe.partition(":")           # ("name:scale": another scale than the recipe's own)
        scale = float(scale) if scale else D_SCALES[name]
        if name == "noiseless":
            out["Lr"] = out["Lr"] * scale
        elif name == "shifted":
            out["r"] = out["r"] + scale
            out["x"] = out["x"] + scale
        else:
            assert name == "diffuse"
            out["L0"] = out["L0"] * scale
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    cache = {}
    with np.load(_PATH) as z:
        for name in z.files:
            c, k = name.split("/")
            a = z[name]
            a.setflags(write=False)
            cache.setdefault(c, {})[k] = a
    return cache


def golden(key):
    """{name: float64 array} of a narrow group-A case: the inputs NAMES, "g_" + name, log_prob, filter_mean, filter_cov"""
    assert key[0] == "A" and key[2:] == A_WIDTHS[0]
    return _golden()[key[1]]


def leaves(key, dtype, device, requires_grad=False):
    return {k: torch.tensor(v, dtype=dtype, device=device, requires_grad=requires_grad) for k, v in inputs(key).items()}


def parts(t):
    """(m0, P0, F, q, Q, H, r, R) in the kernels' layouts from the leaves: covariances from the lower triangles"""
    def cov(L):
        L = L.tril()
        return L @ L.transpose(-1, -2)
    return (t["m0"], cov(t["L0"]), t["F"], t["q"], cov(t["Lq"]), t["H"], t["r"], cov(t["Lr"]))


def model(p, T, B=None):
    """the distribution over the parts; ``B``: its batch shape made (B,) when only a covariance carries the series
    axis (the class derives its batch shape from the locations and matrices, which its constructor keeps in step)"""
    d = dist.GaussianHMM._from_parts(tuple(p), T, None)
    return d if B is None or d.batch_shape == (B,) else d.expand((B,))


@functools.lru_cache(maxsize=None)
def noise(key):
    """(eps [S, B, T, h] for the posterior paths; (e0, ez, ex) for the prior draws: zero noise, then SEEDED draws),
    float64"""
    t = inputs(key)
    (B, T, o), h = t["x"].shape, t["m0"].shape[-1]
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                              # noqa: E731
    eps = r(SEEDED, B, T, h)
    prior = tuple(torch.cat([torch.zeros(1, *s), r(SEEDED, *s)]) for s in ((B, h), (B, T, h), (B, T, o)))
    return eps, prior


def prior_states_model(p, T, B):
    """the model whose x is the z of ``p``: identity observation matrix, no observation noise (r carries the batch)"""
    m0, P0, F, q, Q = p[:5]
    h = m0.shape[-1]
    eye = torch.eye(h, dtype=m0.dtype, device=m0.device)
    return model((m0, P0, F, q, Q, eye[None, None], torch.zeros(B, 1, h, dtype=m0.dtype, device=m0.device),
                  eye[None, None]), T, B)


def _np(v):
    return v.detach().cpu().double().numpy()


def torch_route(t, key_noise, grads=True):
    """Everything the kernels compute, by the torch route of distributions/hmm.py on the leaves' device and dtype ->
    {"log_prob", "g_" + name (leaves' shapes), "filter_mean", "filter_cov", "c", "G", "L", "draws", "prior_x",
    "prior_z"} as float64 numpy arrays"""
    eps, prior = key_noise
    dtype, device = t["x"].dtype, t["x"].device
    eps = eps.to(dtype).to(device)
    prior = [e.to(dtype).to(device) for e in prior]
    B, T, _ = t["x"].shape
    out = {}
    if grads:
        lp = model(parts(t), T, B).log_prob(t["x"])
        for k, g in zip(NAMES, torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])):
            out["g_" + k] = _np(g)
    with torch.no_grad():
        p = parts(t)
        d = model(p, T, B)
        out["log_prob"] = _np(d.log_prob(t["x"]))
        post = d.filter(t["x"])
        out["filter_mean"], out["filter_cov"] = _np(post.loc), _np(post.covariance_matrix)
        maps = hmm._backward_sample_maps(*p, t["x"])
        out["c"], out["G"], out["L"] = (_np(m) for m in maps)
        out["draws"] = _np(hmm._backward_sample(*maps, eps))
        S = prior[0].shape[0]
        out["prior_x"] = _np(d.rsample((S,), noise=prior))
        out["prior_z"] = _np(prior_states_model(p, T, B).rsample((S,), noise=(prior[0], prior[1],
                                                                             torch.zeros_like(prior[1]))))
    return out


@functools.lru_cache(maxsize=None)
def cpu_route(key, dtype):
    """torch_route of the case on the CPU in ``dtype``: float64 is the target, float32 the base of the 4x rule"""
    return torch_route(leaves(key, dtype, CPU, requires_grad=True), noise(key))


def lp_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / (1 + np.abs(want))))


GROUPS = {"grad": tuple("g_" + k for k in NAMES), "filter": ("filter_mean", "filter_cov"), "maps": ("c", "G", "L"),
          "draws": ("draws",), "prior_x": ("prior_x",), "prior_z": ("prior_z",)}


def errors(got, want):
    """{kind: error} over the kinds present in ``got``: log_prob per element |d| / (1 + |want|), every other kind the
    worst gaussian_hmm_cases.rel_err of its arrays.  A NaN anywhere in ``got`` makes its kind's error inf."""
    err = {}
    if "log_prob" in got:
        err["log_prob"] = lp_err(got["log_prob"], want["log_prob"])
    for kind, names in GROUPS.items():
        if all(n in got for n in names):
            err[kind] = max(gc.rel_err(got[n], want[n]) for n in names)
    return {k: (v if np.isfinite(v) else float("inf")) for k, v in err.items()}


# ---- bad pivots that only the backward sweep or the factors see ---------------------------------------------------
# every parameter per-series (series 1 gets the bad matrix); Q time-homogeneous (step_q) and per-step (hom_q)
E_KEYS = tuple(("A", lay, h, o) for lay in ("step_q", "hom_q") for h, o in A_WIDTHS)
E_LONG_T, E_LONG_BAD_STEP = 70, 66


def bad_pivot_parts(key, which, dtype, device):
    """(the eight parts, x) of the case with series 1's Q lowered by 0.55 I ("Q": not positive definite, the innovation
    covariance still is since R >= 0.5 I) or its P0 set to -0.05 I ("P0": the first P^p = Q - 0.05 F^T F still is
    positive definite), or unchanged (None)"""
    t = leaves(key, dtype, device)
    p = [a.clone().contiguous() for a in parts(t)]
    eye = torch.eye(p[0].shape[-1], dtype=dtype, device=device)
    if which == "Q":
        p[4][1] -= 0.55 * eye
    elif which == "P0":
        p[1][1] = -0.05 * eye
    else:
        assert which is None
    return p, t["x"]


@functools.lru_cache(maxsize=None)
def long_draw_inputs(h, o):
    """B = 3, T = 70, every parameter per-series and per-step: the draw kernel's flag scan past one wave of steps"""
    out = make_inputs(np.random.default_rng([20241021, h, o]), 3, E_LONG_T, h, o, (True,) * 6, (True,) * 6)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- batch plumbing through the class ------------------------------------------------------------------------------
C_T = 4
C_SHAPES = ((3, 2), (9, 2))
C_NAMES = ("m0", "L0", "Ft", "q", "Lq", "H", "r", "Lr", "xx")


@functools.lru_cache(maxsize=None)
def class_inputs(h, o, kind="base"):
    """Leaves of batch shape (2, 3): m0 of batch (3,), L0 of (2, 1), F [T, h, h] STORED TRANSPOSED ("Ft"), q of
    (2, 1, 1), Lq of (1, 3, T), H unbatched, r of (2, 3, T), Lr unbatched, and the data as every second step of "xx"
    [2, 3, 2 T, o].  ``kind`` "one": nothing batched but the step axes, batch shape () -- B = 1; "partly": F of batch
    (2, 1) and H of batch (1, 3, 1) as well -- the two parameters the constructor does not broadcast, so the only leads
    that are partly 1 when they reach GaussianHMM._kernel_parts."""
    T = C_T
    one = kind == "one"
    rng = np.random.default_rng([20241022, h, o, ("base", "one", "partly").index(kind)])

    def randn(*shape):
        return rng.standard_normal(shape)

    def tril(shape, n):
        A = randn(*(shape + (n, n)))
        return np.linalg.cholesky(A @ np.swapaxes(A, -1, -2) / n + 0.5 * np.eye(n))

    b = (lambda *s: ()) if one else (lambda *s: s)
    F = randn(*(((2, 1) if kind == "partly" else ()) + (T, h, h)))
    F = F * (0.9 / np.linalg.norm(F, ord=2, axis=(-2, -1)))[..., None, None]
    H = randn(*(((1, 3, 1) if kind == "partly" else ()) + (h, o))) / np.sqrt(h)
    out = {"m0": 0.3 * randn(*b(3), h), "L0": tril(b(2, 1), h), "Ft": np.ascontiguousarray(np.swapaxes(F, -1, -2)),
           "q": 0.3 * randn(*(b(2, 1) + (1, h))), "Lq": tril(b(1, 3) + (T,), h), "H": H,
           "r": 0.3 * randn(*(b(2, 3) + (T, o))), "Lr": tril((), o), "xx": 2.0 * randn(*(b(2, 3) + (2 * T, o)))}
    for a in out.values():
        a.setflags(write=False)
    return out


def class_leaves(h, o, kind, dtype, device, requires_grad=True):
    return {k: torch.tensor(v, dtype=dtype, device=device, requires_grad=requires_grad)
            for k, v in class_inputs(h, o, kind).items()}


def class_build(t):
    """(the GaussianHMM of ``class_leaves`` through its constructor, the data: a [::2] slice on the time axis)"""
    d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["Ft"].transpose(-1, -2),
                         dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                         dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]))
    return d, t["xx"][..., ::2, :]


def class_noise(shape, T, h, o, seed):
    """(noise of rsample_posterior, the triple of rsample) for draws of shape ``shape`` = sample shape + batch, float64"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                              # noqa: E731
    return r(*shape, T, h), (r(*shape, h), r(*shape, T, h), r(*shape, T, o))


def fmt(err):
    return " ".join("%s %.1e" % (k, v) for k, v in err.items())
