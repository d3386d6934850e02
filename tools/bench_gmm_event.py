"""Event-shaped mixtures (``Fam(p0[z], p1[z]).to_event(1)`` with z enumerated) in f32: one
TraceEnum_ELBO.loss_and_grads through the leaf (csrc/mixture_event.hip) against the generic contraction, and the leaf
kernel's own time (developer tool).

    python tools/bench_gmm_event.py [--cases FAMILY:N:K:D,...] [--generic-cap SECONDS]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_gmm_event.py --kernel-only

Per case: milliseconds per loss_and_grads (median of 5 blocks of 5 calls after 3 warm-up calls; each block ends with
a device synchronisation, so a number covers the host work, every launch and the device time of one call), peak
device memory of one call above what was allocated before it, and the leaf call alone (its four kernels, the
workspace allocation and the wrapper) timed the same way, with the rate of (n, k, d) elements it covers per second
(each is visited in the lse pass and twice in the stats pass).  The generic path is timed once first; if that call
takes longer than --generic-cap seconds it is not repeated and the single call is reported.  An out-of-memory error
is reported as such.  Validation is off (its support checks allocate masks of the data's size on either path)."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
from pyro_amd import kernels  # noqa: E402
from pyro_amd.infer import TraceEnum_ELBO  # noqa: E402
from pyro_amd.ops import contract  # noqa: E402
from tests.event_mixture_cases import dist_id, family_params, make_mixture  # noqa: E402

CASES = "Bernoulli:100000:16:784,Poisson:1000000:16:64,Normal:1000000:16:64,Bernoulli:100000:64:784"


def blocks(fn, warm=3, nblk=5, per=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0 = time.perf_counter()
        for _ in range(per):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per)
    return statistics.median(ts)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def elbo_call(leaf, model, guide, x):
    contract.FUSED_MIXTURE = leaf
    elbo = TraceEnum_ELBO(max_plate_nesting=1)
    return lambda: elbo.loss_and_grads(model, guide, x)


def leaf_args(family, x, K, D):
    g = torch.Generator().manual_seed(0)
    p0, p1 = family_params(family, K, D, g)
    a = torch.log_softmax(torch.randn(1, K, generator=g), -1)
    cast = lambda t: None if t is None else t.to(x.device, x.dtype)[None].contiguous()  # noqa: E731
    return dist_id(family), x, a.to(x.device), cast(p0), cast(p1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--generic-cap", type=float, default=5.0)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0],) + tuple(int(v) for v in c.split(":")[1:]) for c in args.cases.split(",")]
    pyro.enable_validation(False)
    for family, N, K, D in cases:
        pyro.clear_param_store()
        model, guide, x = make_mixture(family, N, K, D, torch.float32, dev)
        xa = leaf_args(family, x, K, D)
        if args.kernel_only:        # the leaf alone, 20 calls per case: for rocprofv3 --kernel-trace --stats
            for _ in range(20):
                kernels.mixture_event_fwd_bwd(*xa)
            torch.cuda.synchronize()
            print("%s N=%d K=%d D=%d: 20 leaf calls" % (family, N, K, D), flush=True)
            continue
        pyro.set_rng_seed(0)
        leaf = elbo_call(True, model, guide, x)
        leaf()
        t_leaf = blocks(leaf)
        m_leaf = peak_of(leaf)
        t_k = blocks(lambda: kernels.mixture_event_fwd_bwd(*xa), per=10)
        rate = 3.0 * N * K * D / t_k
        gen = elbo_call(False, model, guide, x)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen()
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            if first > args.generic_cap:
                t_gen, note = first, "one call (over the %.0f s cap)" % args.generic_cap
            else:
                t_gen, note = blocks(gen), ""
            m_gen = "%.0f" % peak_of(gen)
            t_gen = "%.2f" % (t_gen * 1e3)
        except torch.cuda.OutOfMemoryError:
            t_gen, m_gen, note = "OOM", "OOM", "out of device memory"
        contract.FUSED_MIXTURE = True
        del gen
        torch.cuda.empty_cache()
        print("%-9s N=%7d K=%2d D=%4d  leaf %8.3f ms %7.0f MB | leaf call alone %8.3f ms, %6.1f G elem/s | generic "
              "%s ms %s MB %s" % (family, N, K, D, t_leaf * 1e3, m_leaf, t_k * 1e3, rate / 1e9, t_gen, m_gen, note),
              flush=True)
        del model, guide, x, xa
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
