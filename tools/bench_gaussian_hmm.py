"""One log_prob + backward of a GaussianHMM (developer tool): B = 1024 series, T = 512 steps, hidden 8, obs 4, f32,
time-homogeneous parameters shared by the series, by the kernel (csrc/gaussian_hmm.hip: one launch runs the Kalman
filter and the smoother that is its gradient) and with ``hmm.FUSED_GAUSSIAN_HMM = False`` in the same tree (the
sequential torch filter of distributions/hmm.py, differentiated by autograd).

    python tools/bench_gaussian_hmm.py [--shape B:T:H:O] [--dtype f32|f64]

Per route: milliseconds per log_prob(x).sum().backward() as the median of 5 blocks after one warm-up call (one call
per block on the torch route, ten on the kernel's), with the fastest and slowest block; each block ends with a device
synchronisation, so a number covers the host work, every launch and the device time.  Peak memory: what torch's
allocator held at most during one call, above what the inputs occupy.  The two routes' values are compared."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd.distributions import hmm  # noqa: E402


def blocks(fn, per, warm=1, nblk=5):
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


def inputs(B, T, h, o, dtype, dev):
    """the recipe of tests/golden/make_golden_gaussian_hmm.py"""
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                    # noqa: E731

    def tril(n):
        A = r(n, n)
        return torch.linalg.cholesky(A @ A.T / n + 0.5 * torch.eye(n, dtype=torch.float64))
    F = r(h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))
    t = {"m0": 0.3 * r(h), "L0": tril(h), "F": F, "q": 0.3 * r(h), "Lq": tril(h), "H": r(h, o) / h ** 0.5,
         "r": 0.3 * r(o), "Lr": tril(o)}
    t = {k: v.to(dtype).to(dev).requires_grad_() for k, v in t.items()}
    return t, (2.0 * r(B, T, o)).to(dtype).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1024:512:8:4")
    ap.add_argument("--dtype", default="f32", choices=("f32", "f64"))
    args = ap.parse_args()
    B, T, h, o = (int(v) for v in args.shape.split(":"))
    dtype = torch.float32 if args.dtype == "f32" else torch.float64
    dev = torch.device("cuda:0")
    t, x = inputs(B, T, h, o, dtype, dev)
    leaves = list(t.values())

    def one():
        d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                             dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                             dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), validate_args=False)
        lp = d.log_prob(x)
        grads = torch.autograd.grad(lp.sum(), leaves)
        return lp.detach(), grads

    out = {"shape": [B, T, h, o], "dtype": args.dtype}
    values = {}
    for name, fused in (("kernel", True), ("torch", False)):
        hmm.FUSED_GAUSSIAN_HMM = fused
        try:
            med, lo, hi = blocks(one, 10 if fused else 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            values[name] = one()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            hmm.FUSED_GAUSSIAN_HMM = True
        out[name + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        out[name + "_peak_mib"] = round(peak / 2 ** 20, 1)
    out["speedup"] = round(out["torch_ms"]["median"] / out["kernel_ms"]["median"], 1)
    lk, lt = values["kernel"][0].double(), values["torch"][0].double()
    out["log_prob_rel_diff"] = float(((lk - lt).abs() / (1 + lt.abs())).max())
    out["grad_rel_diff"] = max(float((a.double() - b.double()).abs().max() / (1 + b.double().abs().max()))
                               for a, b in zip(values["kernel"][1], values["torch"][1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
