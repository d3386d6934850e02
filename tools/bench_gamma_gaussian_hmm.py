"""One log_prob + backward of a GammaGaussianHMM (developer tool): B = 1024 series, T = 512 steps, hidden 8, obs 4,
time-homogeneous parameters shared by the series, one Gamma per series, in f32 and f64, three ways in one run:

    t_kernel   the Student-t variant of csrc/gaussian_hmm.hip (one launch: the filter at unit scale, then the adjoint
               sweep at covariances divided by the series' weight), through the class
    t_torch    the same class with ``hmm.FUSED_GAUSSIAN_HMM = False`` (the sequential torch filter of
               distributions/hmm.py, differentiated by autograd)
    gaussian   GaussianHMM's log_prob + backward at the same shape and inputs, by its kernel -- what the t kernel is
               expected to cost, plus the scaling

    python tools/bench_gamma_gaussian_hmm.py [--shape B:T:H:O] [--dtypes f32,f64] [--no-torch]

Per route: milliseconds per log_prob(x).sum().backward() as the median of 5 blocks after one warm-up call (one call
per block on the torch route, ten on the kernels'), with the fastest and slowest block; each block ends with a device
synchronisation, so a number covers the host work, every launch and the device time.  ``t_over_gaussian``: the ratio
of the two kernels' medians, and whether the t kernel's median is within the Gaussian figure's own fastest-slowest
spread plus 5 %.  The two t routes' values are compared."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import pyro_amd.distributions as dist  # noqa: E402
from bench_gaussian_hmm import blocks, inputs  # noqa: E402
from pyro_amd.distributions import hmm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1024:512:8:4")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch route (seconds per call at the default shape)")
    args = ap.parse_args()
    B, T, h, o = (int(v) for v in args.shape.split(":"))
    dev = torch.device("cuda:0")
    for name in args.dtypes.split(","):
        dtype = {"f32": torch.float32, "f64": torch.float64}[name]
        t, x = inputs(B, T, h, o, dtype, dev)
        gen = torch.Generator().manual_seed(1)
        t["a"] = (1.0 + 3.0 * torch.rand(B, generator=gen, dtype=torch.float64)).to(dtype).to(dev).requires_grad_()
        t["b"] = (0.5 + 2.5 * torch.rand(B, generator=gen, dtype=torch.float64)).to(dtype).to(dev).requires_grad_()
        leaves = list(t.values())

        def parts():
            return (dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                    dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                    dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]))

        def student():
            d = dist.GammaGaussianHMM(dist.Gamma(t["a"], t["b"], validate_args=False), *parts(), validate_args=False)
            lp = d.log_prob(x)
            return lp.detach(), torch.autograd.grad(lp.sum(), leaves)

        def gaussian():
            lp = dist.GaussianHMM(*parts(), validate_args=False).log_prob(x)
            return lp.detach(), torch.autograd.grad(lp.sum(), leaves[:8])

        out = {"shape": [B, T, h, o], "dtype": name}
        values = {}
        for route, fn, fused in (("t_kernel", student, True), ("gaussian", gaussian, True), ("t_torch", student, False)):
            if route == "t_torch" and args.no_torch:
                continue
            hmm.FUSED_GAUSSIAN_HMM = fused
            try:
                med, lo, hi = blocks(fn, 10 if fused else 1)
                values[route] = fn()
                torch.cuda.synchronize()
            finally:
                hmm.FUSED_GAUSSIAN_HMM = True
            out[route + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        g = out["gaussian_ms"]
        out["t_over_gaussian"] = round(out["t_kernel_ms"]["median"] / g["median"], 4)
        out["within_spread_plus_5pct"] = bool(out["t_kernel_ms"]["median"] <= g["median"] * 1.05 + (g["max"] - g["min"]))
        if "t_torch" in values:
            out["speedup"] = round(out["t_torch_ms"]["median"] / out["t_kernel_ms"]["median"], 1)
            lk, lt = values["t_kernel"][0].double(), values["t_torch"][0].double()
            out["log_prob_rel_diff"] = float(((lk - lt).abs() / (1 + lt.abs())).max())
            out["grad_rel_diff"] = max(float((u.double() - v.double()).abs().max() / (1 + v.double().abs().max()))
                                       for u, v in zip(values["t_kernel"][1], values["t_torch"][1]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
