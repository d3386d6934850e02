"""One LinearHMM.rsample under no_grad (developer tool): S sample paths of the observations of B series of T steps,
hidden 8, obs 4, time-homogeneous matrices shared by the series, Normal initial noise and StudentT transition and
observation noise, at the two shapes
    B = 1024, T = 512, S = 16      (many series, a few draws each)
    B = 1,    T = 512, S = 1024    (one series, many draws)
in f32 and f64, by the kernel (csrc/linear_hmm.hip: one launch, one lane per draw) and with
``hmm.FUSED_LINEAR_HMM = False`` in the same tree (the same-tree baseline: the loop in torch ops of
distributions/hmm.py, the reference's _linear_integrate).

    python tools/bench_linear_hmm.py [--shape B:T:H:O:S ...] [--dtype f32|f64 ...]

Per route: milliseconds per call (noise drawn inside the call by the three components' rsample, as a user's call does)
as the median of 5 blocks after one warm-up call (one call per block on the torch route, ten on the kernel's), with the
fastest and slowest block; each block ends with a device synchronisation, so a number covers the host work, the noise
draws, every launch and the device time.  Peak memory: what torch's allocator held at most during one call, above what
the inputs occupy.

The kernel's own time comes from device events around kernels.linear_hmm_draw with given noise, 5 blocks of ten:
median, fastest and slowest.  Beside it, measured the same way in the same process at the same shape and dtype, the
draw kernel of csrc/gaussian_hmm_draw.hip with shared time-homogeneous Gaussian parameters (its full call minus a call
with T = 1, S = 1, which runs the same factors kernel): per step it computes what this kernel computes plus L_Q e,
L_R e', q and r, and it moves the same noise in and the same y out, so it is the yardstick.  ``kernel_gbps``: the
achieved rate counting the noise read plus y written.  One line of JSON per shape and dtype."""
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
    return ts


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def inputs(B, h, o, dtype, dev):
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                    # noqa: E731
    F = r(h, h)
    F = F * (0.9 / torch.linalg.matrix_norm(F, ord=2))
    t = {"m0": 0.3 * r(B, h), "s0": 0.5 + torch.rand(h, generator=gen, dtype=torch.float64), "F": F,
         "q": 0.3 * r(h), "sq": 0.5 + torch.rand(h, generator=gen, dtype=torch.float64), "H": r(h, o) / h ** 0.5,
         "r": 0.3 * r(o), "sr": 0.5 + torch.rand(o, generator=gen, dtype=torch.float64)}
    return {k: v.to(dtype).to(dev) for k, v in t.items()}


def one_shape(B, T, h, o, S, name, dev):
    dtype = torch.float32 if name == "f32" else torch.float64
    t = inputs(B, h, o, dtype, dev)
    df = torch.tensor(3.0, dtype=dtype, device=dev)
    d = dist.LinearHMM(dist.Normal(t["m0"], t["s0"]).to_event(1), t["F"],
                       dist.StudentT(df, t["q"], t["sq"]).to_event(1), t["H"],
                       dist.StudentT(df, t["r"], t["sr"]).to_event(1), duration=T)

    def one(noise=None):
        with torch.no_grad():
            return d.rsample((S,), noise=noise)

    out = {"shape": {"B": B, "T": T, "hidden": h, "obs": o, "S": S}, "dtype": name}
    for route, fused in (("kernel", True), ("same_tree_torch", False)):
        hmm.FUSED_LINEAR_HMM = fused
        try:
            med, lo, hi = blocks(one, 10 if fused else 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            one()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            hmm.FUSED_LINEAR_HMM = True
        out[route + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        out[route + "_peak_mib"] = round(peak / 2 ** 20, 1)
    out["speedup"] = round(out["same_tree_torch_ms"]["median"] / out["kernel_ms"]["median"], 1)
    # the noise draws alone: what both routes spend before the chain
    with torch.no_grad():
        draws = lambda: (d.initial_dist.rsample((S,)), d.transition_dist.expand((B, T)).rsample((S,)),      # noqa: E731
                         d.observation_dist.expand((B, T)).rsample((S,)))
        out["noise_draws_ms"] = round(blocks(draws, 10)[0], 3)
        noise = draws()
    # the two routes on one noise triple
    yk = one(noise).double()
    hmm.FUSED_LINEAR_HMM = False
    try:
        yt = one(noise).double()
    finally:
        hmm.FUSED_LINEAR_HMM = True
    out["draws_rel_diff"] = float((yk - yt).abs().max() / (1 + yt.abs().max()))
    # the kernel's own time, and the Gaussian draw kernel's at the same shape
    Fk, Hk = t["F"].reshape(1, 1, h, h), t["H"].reshape(1, 1, h, o)
    flat = [e.reshape((S, B) + tuple(e.shape[2:])).contiguous() for e in noise]
    ts = device_ms(lambda: kernels.linear_hmm_draw(Fk, Hk, T, *flat))
    out["kernel_device_ms"] = stats(ts)
    nbytes = (sum(e.numel() for e in flat) + S * B * T * o) * flat[0].element_size()
    out["kernel_gbps"] = round(nbytes / statistics.median(ts) / 1e6, 1)
    g = dist.GaussianHMM(dist.Normal(t["m0"], t["s0"]).to_event(1), t["F"], dist.Normal(t["q"], t["sq"]).to_event(1),
                         t["H"], dist.Normal(t["r"], t["sr"]).to_event(1), validate_args=False, duration=T)
    args = g._kernel_parts(g.batch_shape)
    eps = [torch.randn_like(e) for e in flat]
    tiny = [e[:1, :, :1].contiguous() if e.dim() == 4 else e[:1].contiguous() for e in eps]
    factors = statistics.median(device_ms(lambda: kernels.gaussian_hmm_draw(*args, 1, *tiny)))
    both = device_ms(lambda: kernels.gaussian_hmm_draw(*args, T, *eps))
    out["gaussian_factors_ms"] = round(factors, 3)
    out["gaussian_draw_device_ms"] = stats([b - factors for b in both])
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
