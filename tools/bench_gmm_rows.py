"""Mixtures with per-row assignment weights (a gating network: ``z_n ~ Categorical(logits=X_n @ W + b)``, z enumerated)
in f32: one TraceEnum_ELBO.loss_and_grads with the mixture leaves on (csrc/mixture_rows.hip where the package has it)
and with ``contract.FUSED_MIXTURE = False`` (developer tool).  Public interface only: the same file runs on a commit
without the per-row leaf, where both columns are the generic contraction -- the baseline.

    python tools/bench_gmm_rows.py [--cases N:K:D[:detached],...]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_gmm_rows.py --profile

D = 0: scalar Normal observations; D > 0: a diagonal Normal over D features; ``detached``: the gate's logits carry no
gradient (the leaf then writes no responsibilities).  Per case: milliseconds per loss_and_grads (median of 5 blocks of
5 calls after 3 warm-up calls; each block ends with a device synchronisation, so a number covers the host work, every
launch and the device time of one call) and peak device memory of one call above what was allocated before it, for
both settings.  --profile: 20 calls per case with the leaves on and nothing else, for the kernel times of
``rocprofv3 --kernel-trace --stats`` (the per-row kernels are mixture_rows_kernel / mixture_rows_diag_kernel; their
algorithmic traffic is N (2 K + 1) sizeof(T) bytes for scalar data -- a read, the responsibilities written, x read).
Validation is off (its support checks allocate masks of the data's size on either path)."""
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
from torch.distributions import constraints  # noqa: E402

CASES = "1000000:16:0,1000000:16:8,1000000:16:0:detached"
F = 8          # gate features


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


def make_experts(N, K, D, detached, dev):
    g = torch.Generator().manual_seed(0)
    shape = (K,) if D == 0 else (K, D)
    centres = 3.0 * torch.randn(*shape, generator=g)
    z = torch.randint(0, K, (N,), generator=g)
    x = (centres[z] + torch.randn(N, *shape[1:], generator=g)).to(dev)
    X = torch.randn(N, F, generator=g).to(dev)
    W0, loc0 = (0.3 * torch.randn(F, K, generator=g)).to(dev), (centres + 0.3 * torch.randn(*shape, generator=g)).to(dev)

    def model(x):
        W = pyro.param("W", W0.clone())
        b = pyro.param("b", torch.zeros(K, device=dev))
        loc = pyro.param("loc", loc0.clone())
        scale = pyro.param("scale", torch.ones(*shape, device=dev), constraint=constraints.positive)
        with pyro.plate("data", N):
            logits = X @ W + b
            zz = pyro.sample("z", dist.Categorical(logits=logits.detach() if detached else logits),
                             infer={"enumerate": "parallel"})
            d = dist.Normal(loc[zz], scale[zz])
            pyro.sample("x", d.to_event(1) if D else d, obs=x)

    return model, (lambda x: None), x


def elbo_call(leaf, model, guide, x):
    elbo = TraceEnum_ELBO(max_plate_nesting=1)

    def call():
        contract.FUSED_MIXTURE = leaf
        try:
            return elbo.loss_and_grads(model, guide, x)
        finally:
            contract.FUSED_MIXTURE = True
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pyro.enable_validation(False)
    for case in args.cases.split(","):
        parts = case.split(":")
        N, K, D = (int(v) for v in parts[:3])
        detached = len(parts) > 3 and parts[3] == "detached"
        pyro.clear_param_store()
        model, guide, x = make_experts(N, K, D, detached, dev)
        leaf = elbo_call(True, model, guide, x)
        tag = "N=%7d K=%2d D=%d%s" % (N, K, D, " detached" if detached else "")
        if args.profile:
            for _ in range(20):
                leaf()
            torch.cuda.synchronize()
            print("%s: 20 calls" % tag, flush=True)
            continue
        loss_on = leaf()
        t_on, m_on = blocks(leaf), peak_of(leaf)
        gen = elbo_call(False, model, guide, x)
        loss_off = gen()
        t_off, m_off = blocks(gen), peak_of(gen)
        print("%-28s leaves on %8.3f ms %6.0f MB (loss %.6g) | FUSED_MIXTURE = False %8.3f ms %6.0f MB (loss %.6g)" % (
            tag, t_on * 1e3, m_on, loss_on, t_off * 1e3, m_off, loss_off), flush=True)
        del model, guide, x, leaf, gen
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
