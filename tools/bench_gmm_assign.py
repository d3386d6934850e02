"""Asking a fitted mixture for its clustering, N = 1e6 rows, K = 16 components, f32 (developer tool): infer_discrete at
temperature 0 and 1 with the assignment kernel (csrc/mixture_assign.hip) and with ``contract.FUSED_MIXTURE = False``
(the generic route), and -- for temperature 1 -- TraceEnum_ELBO.sample_posterior on the same model, the only route the
package had before.  Public interface only: on a commit without infer_discrete the file prints the sample_posterior
column alone -- the baseline.

    python tools/bench_gmm_assign.py [--cases N:K:D,...]

D = 0: scalar Normal observations; D > 0: a diagonal Normal over D features.  Per case and route: milliseconds per
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

CASES = "1000000:16:0,1000000:16:8"


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


def with_leaf(leaf, fn):
    def call():
        contract.FUSED_MIXTURE = leaf
        try:
            return fn()
        finally:
            contract.FUSED_MIXTURE = True
    return call


def report(tag, route, fn):
    z = fn()
    assert z.shape[-1] == int(tag.split()[0].split("=")[1]) and z.dtype == torch.int64
    (med, lo, hi), mem = blocks(fn), peak_of(fn)
    print("%-22s %-42s %9.3f ms (blocks %9.3f .. %9.3f) %7.0f MB" % (tag, route, med, lo, hi, mem), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pyro.enable_validation(False)
    for case in args.cases.split(","):
        N, K, D = (int(v) for v in case.split(":"))
        model, x = make_mixture(N, K, D, dev)
        tag = "N=%d K=%d D=%d" % (N, K, D)
        if infer_discrete is not None:
            for temperature in (0, 1):
                fn = infer_discrete(model, first_available_dim=-2, temperature=temperature)
                report(tag, "infer_discrete T=%d, assignment kernel" % temperature, with_leaf(True, lambda: fn(x)))
                report(tag, "infer_discrete T=%d, FUSED_MIXTURE = False" % temperature,
                       with_leaf(False, lambda: fn(x)))
        elbo = TraceEnum_ELBO(max_plate_nesting=1)
        report(tag, "sample_posterior (T=1)", lambda: elbo.sample_posterior(model, lambda x: None, x))
        del model, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
