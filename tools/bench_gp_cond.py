"""The per-point marginals of VariationalSparseGP under a gradient by the two routes of the same tree (developer tool;
not part of bench.py):
    streamed  csrc/gp_cond.hip: loc and s in one pass over X, their gradient in two more, Kuf never in memory
    dense     ``util.conditional(X, Xu, kernel, u_loc, u_scale_tril, Luu, full_cov=False)`` and autograd (the baseline)

    python tools/bench_gp_cond.py [--iters 5] [--min-n 0] [--max-n 100000]

Forward plus backward of sum(loc w) + sum(var v) with respect to Xu, the kernel's parameters, u_loc and u_scale_tril,
RBF with ARD lengthscales, D = 8, ``whiten=True``, for N in {1e3, 1e4, 1e5}, M in {64, 256}, Q in {1, 8}, f32 and f64.
A float32 model stays on the dense route (``VariationalSparseGP._streamed``), so both of its columns are the dense
route; its kernels-alone columns are the f32 (MFMA) kernels.  Per route: milliseconds per step as the median of 5 blocks after one warm-up block with the fastest
and slowest block, and the allocator's peak above what the inputs hold (tools/bench_gp_kernel.py's ``blocks`` and
``peak_mib``).  The three kernels alone are timed by device events in the dtype named.  One line of JSON per case."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.contrib.gp as gp  # noqa: E402
from bench_gp_kernel import blocks, data, peak_mib  # noqa: E402
from bench_gp_sgpr import events_ms  # noqa: E402
from pyro_amd import kernels  # noqa: E402


def case(N, M, Q, dtype, iters, dev):
    X, _ = data(N, 8, dtype, dev)
    pyro.clear_param_store()
    kern = gp.kernels.RBF(8, variance=torch.tensor(1.0, dtype=dtype), lengthscale=torch.ones(8, dtype=dtype)).to(dev)
    Xu = X[::max(N // M, 1)][:M].clone()
    y = torch.zeros(Q, N, dtype=dtype, device=dev)
    model = gp.models.VariationalSparseGP(X, y, kern, Xu, gp.likelihoods.Gaussian().to(dev), whiten=True, jitter=1e-4)
    gen = torch.Generator(device=dev).manual_seed(1)
    w, v = (torch.randn(Q, N, generator=gen, dtype=dtype, device=dev) for _ in range(2))

    def step():
        for p in model.parameters():
            p.grad = None
        loc, var = model._marginals(X, model._factor())
        ((loc * w).sum() + (var * v).sum()).backward()

    out = {"case": "vsgp_marginals", "N": N, "M": M, "Q": Q, "D": 8, "dtype": str(dtype).replace("torch.", "")}
    saved = gp.models.FUSED_VSGP_MIN_N
    for route, fused in (("streamed", True), ("dense", False)):
        gp.models.FUSED_VSGP, gp.models.FUSED_VSGP_MIN_N = fused, 0
        try:
            out[route + "_ms"] = blocks(step, iters)
            out[route + "_peak_mib"] = peak_mib(step)
        finally:
            gp.models.FUSED_VSGP, gp.models.FUSED_VSGP_MIN_N = True, saved
    ls, var = torch.ones(8, dtype=dtype, device=dev), torch.ones(1, dtype=dtype, device=dev)
    a, P = torch.randn(M, Q, dtype=dtype, device=dev), torch.randn(Q + 1, M, M, dtype=dtype, device=dev).tril()
    g_loc, g_s = torch.randn(N, Q, dtype=dtype, device=dev), torch.randn(N, Q + 1, dtype=dtype, device=dev)
    gram, chain = (False,) * 5 + (True, True), (False, True, True, True, False, False, False)
    for name, fn in (("fwd", lambda: kernels.gp_cond_fwd(X, Xu, a, P, ls, var)),
                     ("bwd_gram", lambda: kernels.gp_cond_bwd(X, Xu, a, P, ls, var, None, g_loc, g_s, "rbf", gram)),
                     ("bwd_chain", lambda: kernels.gp_cond_bwd(X, Xu, a, P, ls, var, None, g_loc, g_s, "rbf", chain))):
        med, lo, hi = events_ms(fn, iters)
        out["kernel_%s_ms" % name] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=10 ** 5)
    ap.add_argument("--min-n", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for dtype in (torch.float32, torch.float64):
        for N in (10 ** 3, 10 ** 4, 10 ** 5):
            for M in (64, 256):
                for Q in (1, 8):
                    if args.min_n <= N <= args.max_n:
                        case(N, M, Q, dtype, args.iters, dev)


if __name__ == "__main__":
    main()
