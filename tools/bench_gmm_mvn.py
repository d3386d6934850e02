"""The full-covariance Gaussian mixture (MultivariateNormal(locs[z], scale_tril=L[z]) with z enumerated) at
N = 1e6, f32: one TraceEnum_ELBO.loss_and_grads through the leaf (csrc/mixture_mvn.hip) against the generic
contraction, and the leaf kernel's own time (developer tool).

    python tools/bench_gmm_mvn.py [--configs K:D,...] [--generic-cap SECONDS]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_gmm_mvn.py --kernel-only

Per (K, D): milliseconds per loss_and_grads (median of 5 blocks of 5 calls after 3 warm-up calls; each block ends
with a device synchronisation, so a number covers the host work, every launch and the device time of one call),
peak device memory of one call above what was allocated before it, and the leaf call alone (its three kernels,
the workspace allocation and the wrapper) timed the same way, with its fraction of the f32 matrix peak
(157.3 TFLOP/s) at 4 N K D^2 FLOP (2 N K D^2 for z = W d, as many for G).  The generic path is timed once first;
if that call takes longer than --generic-cap seconds it is not repeated and the single call is reported.  An
out-of-memory error, or the failure of torch's batched hipBLAS triangular solve to allocate its workspace, is
reported as such.  --n picks a smaller N at which the generic path runs."""
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
from tests.mvn_mixture_cases import make_gmm  # noqa: E402

PEAK = 157.3e12


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


def leaf_args(K, D, N, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g).to(dev)
    a = torch.log_softmax(torch.randn(1, K, generator=g), -1).to(dev)
    loc = torch.randn(1, K, D, generator=g).to(dev)
    W = (torch.eye(D) + 0.1 * torch.tril(torch.randn(K, D, D, generator=g), -1)).reshape(1, K, D, D).to(dev)
    return x, a, loc, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4:2,4:8,4:32,4:64,16:2,16:8,16:32,16:64,64:2,64:8,64:32,64:64")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--generic-cap", type=float, default=5.0)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.n
    configs = [tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")]
    pyro.enable_validation(False)
    if args.kernel_only:           # the leaf alone, 20 calls per config: for rocprofv3 --kernel-trace --stats
        for K, D in configs:
            xa = leaf_args(K, D, N, dev)
            for _ in range(20):
                kernels.mixture_mvn_fwd_bwd(*xa)
            torch.cuda.synchronize()
            print("K=%d D=%d: 20 leaf calls" % (K, D), flush=True)
        return
    print("N=%d f32; ms per loss_and_grads (median of 5 x 5 after 3), peak MB above the inputs" % N, flush=True)
    for K, D in configs:
        pyro.clear_param_store()
        model, guide, x = make_gmm(N, K, D, torch.float32, dev, form="tril")
        pyro.set_rng_seed(0)
        leaf = elbo_call(True, model, guide, x)
        leaf()
        t_leaf = blocks(leaf)
        m_leaf = peak_of(leaf)
        xa = leaf_args(K, D, N, dev)
        t_k = blocks(lambda: kernels.mixture_mvn_fwd_bwd(*xa), per=10)
        frac = 4.0 * N * K * D * D / t_k / PEAK
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
        except RuntimeError as e:         # (torch's batched hipBLAS triangular solve: its workspace allocation)
            if "ALLOC_FAILED" not in str(e):
                raise
            t_gen, m_gen, note = "failed", "-", "HIPBLAS_STATUS_ALLOC_FAILED in torch's MultivariateNormal.log_prob"
        contract.FUSED_MIXTURE = True
        del gen
        torch.cuda.empty_cache()
        print("K=%2d D=%2d  leaf %8.3f ms %7.0f MB | leaf call alone %8.3f ms, %5.1f%% of f32 peak | generic %s ms "
              "%s MB %s" % (K, D, t_leaf * 1e3, m_leaf, t_k * 1e3, 100 * frac, t_gen, m_gen, note), flush=True)


if __name__ == "__main__":
    main()
