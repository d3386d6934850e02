"""Asking a fitted mixture for its clustering, K = 16 components, f32 (developer tool): infer_discrete at
temperature 0 and 1 with the assignment kernels (csrc/mixture_assign.hip, csrc/mixture_assign_wide.hip) and with
``contract.FUSED_MIXTURE = False``
(the generic route), and -- for temperature 1 -- TraceEnum_ELBO.sample_posterior on the same model, the only route the
package had before.  Public interface only: on a commit without infer_discrete the file prints the sample_posterior
column alone -- the baseline.

    python tools/bench_gmm_assign.py [--cases [bern:|mvn:]N:K:D,...]

D = 0: scalar Normal observations; D > 0: a diagonal Normal over D features; ``bern:`` binarised images under
``Bernoulli(logits=l[z]).to_event(1)``; ``mvn:`` ``MultivariateNormal(locs[z], scale_tril=L[z])`` (for these two the
sample_posterior column is left out, and a route that runs out of device memory is reported as such).  Per case and route: milliseconds per
call as the median of 7 blocks of 3 calls after 2 warm-up calls, with the fastest and slowest block (the run-to-run
spread a difference has to exceed); each block ends with a device synchronisation, so a number covers the host work,
every launch and the device time of one call.  Peak device memory of one call above what was allocated before it, by
torch.cuda.max_memory_allocated.  Validation is off (its support checks allocate masks of the data's size)."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd.infer import TraceEnum_ELBO  # noqa: E402
from pyro_amd.ops import contract  # noqa: E402

try:
    from pyro_amd.infer import infer_discrete
except ImportError:                    # a commit before infer_discrete: the baseline column only
    infer_discrete = None

CASES = "1000000:16:0,1000000:16:8,bern:100000:16:784,mvn:1000000:16:32"


def blocks(fn, warm=2, nblk=7, per=3):
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
    return statistics.median(ts), min(ts), max(ts)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def make_mixture(N, K, D, dev):
    g = torch.Generator().manual_seed(0)
    shape = (K,) if D == 0 else (K, D)
    centres = 3.0 * torch.randn(*shape, generator=g)
    z = torch.randint(0, K, (N,), generator=g)
    x = (centres[z] + torch.randn(N, *shape[1:], generator=g)).to(dev)
    loc = (centres + 0.1 * torch.randn(*shape, generator=g)).to(dev)
    scale = torch.ones(*shape, device=dev)
    pi = torch.softmax(torch.randn(K, generator=g), -1).to(dev)

    def model(x):
        with pyro.plate("data", N):
            zz = pyro.sample("z", dist.Categorical(pi), infer={"enumerate": "parallel"})
            d = dist.Normal(loc[zz], scale[zz])
            pyro.sample("x", d.to_event(1) if D else d, obs=x)
        return zz

    return model, x


def make_wide_mixture(kind, N, K, D, dev):
    g = torch.Generator().manual_seed(0)
    z = torch.randint(0, K, (N,), generator=g)
    pi = torch.softmax(torch.randn(K, generator=g), -1).to(dev)
    if kind == "bern":
        logits = 2.0 * torch.randn(K, D, generator=g)
        x = torch.bernoulli(torch.sigmoid(logits[z]), generator=g).to(dev)
        logits = (logits + 0.1 * torch.randn(K, D, generator=g)).to(dev)
        obs = lambda zz: dist.Bernoulli(logits=logits[zz]).to_event(1)               # noqa: E731
    else:
        centres = 3.0 * torch.randn(K, D, generator=g)
        x = (centres[z] + torch.randn(N, D, generator=g)).to(dev)
        locs = (centres + 0.1 * torch.randn(K, D, generator=g)).to(dev)
        L = torch.tril(0.3 / D ** 0.5 * torch.randn(K, D, D, generator=g), -1) + \
            torch.diag_embed(0.8 + 0.4 * torch.rand(K, D, generator=g))
        L = L.to(dev)
        obs = lambda zz: dist.MultivariateNormal(locs[zz], scale_tril=L[zz])       # noqa: E731

    def model(x):
        with pyro.plate("data", N):
            zz = pyro.sample("z", dist.Categorical(pi), infer={"enumerate": "parallel"})
            pyro.sample("x", obs(zz), obs=x)
        return zz

    return model, x


def with_leaf(leaf, fn):
    def call():
        contract.FUSED_MIXTURE = leaf
        try:
            return fn()
        finally:
            contract.FUSED_MIXTURE = True
    return call


def report(tag, route, fn):
    try:
        z = fn()
        assert z.shape[-1] == int(tag.split()[0].split("=")[1]) and z.dtype == torch.int64
        del z
        (med, lo, hi), mem = blocks(fn), peak_of(fn)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        print("%-22s %-42s OUT OF MEMORY" % (tag, route), flush=True)
        return
    print("%-22s %-42s %9.3f ms (blocks %9.3f .. %9.3f) %7.0f MB" % (tag, route, med, lo, hi, mem), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pyro.enable_validation(False)
    for case in args.cases.split(","):
        kind = case.split(":")[0] if case[0].isalpha() else None
        N, K, D = (int(v) for v in case.split(":")[-3:])
        model, x = make_mixture(N, K, D, dev) if kind is None else make_wide_mixture(kind, N, K, D, dev)
        tag = "N=%d K=%d D=%d%s" % (N, K, D, "" if kind is None else " " + kind)
        if infer_discrete is not None:
            for temperature in (0, 1):
                fn = infer_discrete(model, first_available_dim=-2, temperature=temperature)
                report(tag, "infer_discrete T=%d, assignment kernel" % temperature, with_leaf(True, lambda: fn(x)))
                report(tag, "infer_discrete T=%d, FUSED_MIXTURE = False" % temperature,
                       with_leaf(False, lambda: fn(x)))
        if kind is None:
            elbo = TraceEnum_ELBO(max_plate_nesting=1)
            report(tag, "sample_posterior (T=1)", lambda: elbo.sample_posterior(model, lambda x: None, x))
        del model, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
