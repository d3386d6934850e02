"""One Trace_ELBO.loss_and_grads of a plated regression model per family (developer tool): linear (Normal), robust
(StudentT), count (Poisson, log link) and grouped-trials logistic (Binomial) regression of N = 1e6 rows on D = 32
features in f32, with P = 64 vectorised particles and with P = 1, two ways:

    fused      the observed site is distributions/families.py::_LinearPredictor: one pass of csrc/glm_family.hip over X
    same_tree  ``families.FUSED_GLM_FAMILIES = False``: the same model text on the same tree, the predictor and the
               log-probabilities materialised as [P, N] tensors with their autograd duals

    python tools/bench_glm_family.py [--n N] [--d D] [--particles P ...] [--family NAME ...]

Per route: milliseconds per step (model + AutoNormal guide + backward, eager) as the median of 5 blocks after two
warm-up steps (five steps per block), with the fastest and slowest block; each block ends with a device
synchronisation.  Peak memory: what torch's allocator held at most during one step, above what it held before it.
``loss`` / ``rel_loss_diff``: the two routes' losses on the same draws.  ``kernel_device_ms``: the site's launches
alone (kernels.glm_family_fwd_bwd: the pass over X and its finalize) from device events, median of 5 blocks of ten.
One line of JSON per family and particle count."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd import _lib, kernels  # noqa: E402
from pyro_amd.distributions import families  # noqa: E402
from pyro_amd.infer import Trace_ELBO  # noqa: E402
from pyro_amd.infer.autoguide import AutoNormal  # noqa: E402

FAMILIES = ("normal", "student_t", "poisson", "binomial")


def make_model(family):
    def model(X, y, count=None):
        N, D = X.shape
        w = pyro.sample("w", dist.Normal(X.new_zeros(D), 1.0).to_event(1))
        b = pyro.sample("b", dist.Normal(X.new_zeros(()), 1.0))
        if family in ("normal", "student_t"):
            sigma = pyro.sample("sigma", dist.LogNormal(X.new_zeros(()), 0.5))
        if family == "student_t":
            nu = pyro.sample("nu", dist.Gamma(X.new_full((), 4.0), X.new_full((), 0.5)))
        with pyro.plate("data", N):
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


def make_data(family, N, D, dev):
    g = torch.Generator().manual_seed(0)
    X = torch.randn((N, D), generator=g)
    w = torch.randn((D,), generator=g) / D ** 0.5
    eta = X @ w
    count = None
    if family == "normal":
        y = eta + torch.randn((N,), generator=g)
    elif family == "student_t":
        y = eta + torch.randn((N,), generator=g) / torch.rand((N,), generator=g).clamp_min(0.05).sqrt()
    elif family == "poisson":
        y = torch.poisson(eta.exp(), generator=g)
    else:
        count = torch.randint(1, 21, (N,), generator=g).float()
        y = torch.binomial(count, torch.sigmoid(eta), generator=g)
    return X.to(dev), y.to(dev), (None if count is None else count.to(dev))


def blocks(fn, per=5, warm=2, nblk=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        for _ in range(per):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per * 1e3)
    return {"ms": round(statistics.median(ts), 3), "fastest": round(min(ts), 3), "slowest": round(max(ts), 3)}


def kernel_device_ms(family, X, y, count, P, per=10, nblk=5):
    fid = FAMILIES.index(family)
    g = torch.Generator().manual_seed(1)
    w = (0.05 * torch.randn((P, X.shape[1]), generator=g)).to(X.device)
    b = (0.05 * torch.randn((P,), generator=g)).to(X.device)
    A = _lib.GLM_AUX_COLUMNS[fid]
    aux = (torch.rand((P, A), generator=g) + (3.0 if A == 2 else 0.5)).to(X.device) if A else None

    def fn():
        kernels.glm_family_fwd_bwd(fid, X, y, w, b, aux, count, None, 1.0)

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / per)
    return {"ms": round(statistics.median(ts), 4), "fastest": round(min(ts), 4), "slowest": round(max(ts), 4)}


def run(family, N, D, P, dev):
    X, y, count = make_data(family, N, D, dev)
    model = make_model(family)
    out = {"family": family, "N": N, "D": D, "P": P, "dtype": "f32"}
    out["kernel_device_ms"] = kernel_device_ms(family, X, y, count, P)
    losses = {}
    for route, fused in (("fused", True), ("same_tree", False)):
        families.FUSED_GLM_FAMILIES = fused
        pyro.clear_param_store()
        pyro.set_rng_seed(0)
        guide = AutoNormal(model, init_scale=0.05)
        elbo = Trace_ELBO(num_particles=P, vectorize_particles=P > 1, max_plate_nesting=1)

        def step():
            loss = elbo.loss_and_grads(model, guide, X, y, count)
            for p in pyro.get_param_store()._params.values():
                p.grad = None
            return loss

        pyro.set_rng_seed(1)
        losses[route] = float(step())
        res = blocks(step)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res["peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        out[route] = res
        torch.cuda.empty_cache()
    families.FUSED_GLM_FAMILIES = True
    out["speedup"] = round(out["same_tree"]["ms"] / out["fused"]["ms"], 2)
    out["loss"] = losses
    out["rel_loss_diff"] = abs(losses["fused"] - losses["same_tree"]) / abs(losses["same_tree"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--particles", type=int, nargs="*", default=[64, 1])
    ap.add_argument("--family", nargs="*", default=list(FAMILIES))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for P in args.particles:
        for family in args.family:
            print(json.dumps(run(family, args.n, args.d, P, dev)), flush=True)


if __name__ == "__main__":
    main()
