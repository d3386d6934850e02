"""One GaussianHMM.rsample_posterior under no_grad (developer tool): S draws of the latent path of B series of T steps,
hidden 8, obs 4, time-homogeneous parameters shared by the series, at the two shapes
    B = 1024, T = 512, S = 16      (many series, a few draws each)
    B = 1,    T = 512, S = 1024    (forecasting: one series, many draws)
in f32 and f64, by the kernels (csrc/gaussian_hmm_sample.hip: the maps kernel, one wave per series, then the paths
kernel, one lane per draw) and with ``hmm.FUSED_GAUSSIAN_HMM = False`` in the same tree (the same-tree baseline: the
sequential torch filter and backward-sampling loop of distributions/hmm.py).

    python tools/bench_gaussian_hmm_sample.py [--shape B:T:H:O:S ...] [--dtype f32|f64 ...]

Per route: milliseconds per call (noise drawn inside the call, as a user's call does) as the median of 5 blocks after
one warm-up call (one call per block on the torch route, ten on the kernels'), with the fastest and slowest block;
each block ends with a device synchronisation, so a number covers the host work, every launch and the device time.
Peak memory: what torch's allocator held at most during one call, above what the inputs occupy.

The two kernels' own times come from device events around kernels.gaussian_hmm_sample with a given eps, median of 5
blocks of ten: ``maps_ms`` is a call with S = 0 that keeps the maps (the maps kernel alone), ``paths_ms`` the
full call minus that.  ``paths_gbps``: the paths kernel's achieved rate counting eps read plus z written (the maps it
also reads are B T (h + 2 h^2) elements, re-read by every block of 64 draws, mostly from cache).  One line of JSON per
shape and dtype."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd.distributions as dist  # noqa: E402
from pyro_amd import kernels  # noqa: E402
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


def device_ms(fn, per=10, nblk=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / per)
    return statistics.median(ts)


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
    t = {k: v.to(dtype).to(dev) for k, v in t.items()}
    return t, (2.0 * r(B, T, o)).to(dtype).to(dev)


def one_shape(B, T, h, o, S, name, dev):
    dtype = torch.float32 if name == "f32" else torch.float64
    t, x = inputs(B, T, h, o, dtype, dev)
    d = dist.GaussianHMM(dist.MultivariateNormal(t["m0"], scale_tril=t["L0"]), t["F"],
                         dist.MultivariateNormal(t["q"], scale_tril=t["Lq"]), t["H"],
                         dist.MultivariateNormal(t["r"], scale_tril=t["Lr"]), validate_args=False)

    def one(noise=None):
        with torch.no_grad():
            return d.rsample_posterior(x, (S,), noise=noise)

    out = {"shape": {"B": B, "T": T, "hidden": h, "obs": o, "S": S}, "dtype": name}
    for route, fused in (("kernel", True), ("same_tree_torch", False)):
        hmm.FUSED_GAUSSIAN_HMM = fused
        try:
            med, lo, hi = blocks(one, 10 if fused else 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            one()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            hmm.FUSED_GAUSSIAN_HMM = True
        out[route + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        out[route + "_peak_mib"] = round(peak / 2 ** 20, 1)
    out["speedup"] = round(out["same_tree_torch_ms"]["median"] / out["kernel_ms"]["median"], 1)
    # the two routes on one noise tensor
    noise = torch.randn(S, B, T, h, dtype=dtype, device=dev)
    zk = one(noise).double()
    hmm.FUSED_GAUSSIAN_HMM = False
    try:
        zt = one(noise).double()
    finally:
        hmm.FUSED_GAUSSIAN_HMM = True
    out["draws_rel_diff"] = float((zk - zt).abs().max() / (1 + zt.abs().max()))
    # the kernels' own times
    batch, _ = d._check_value(x)
    args = d._kernel_inputs(x, batch, T)
    eps = noise.reshape(S, B, T, h)
    maps_ms = device_ms(lambda: kernels.gaussian_hmm_sample(*args, eps[:0], need_maps=True))
    both_ms = device_ms(lambda: kernels.gaussian_hmm_sample(*args, eps))
    out["maps_ms"] = round(maps_ms, 3)
    out["paths_ms"] = round(both_ms - maps_ms, 3)
    out["paths_gbps"] = round(2 * eps.numel() * eps.element_size() / max(both_ms - maps_ms, 1e-6) / 1e6, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["1024:512:8:4:16", "1:512:8:4:1024"])
    ap.add_argument("--dtype", nargs="+", default=["f32", "f64"], choices=("f32", "f64"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in args.shape:
        B, T, h, o, S = (int(v) for v in shape.split(":"))
        for name in args.dtype:
            one_shape(B, T, h, o, S, name, dev)


if __name__ == "__main__":
    main()
