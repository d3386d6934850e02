"""SparseGPRegression under a gradient by the two routes of the same tree (developer tool; not part of bench.py):
    streamed  csrc/gp_sgpr.hip: A = Kuf Kuf^T and b = Kuf r in one pass over X each way, Kuf never in memory
    dense     ``models.FUSED_SGPR = False``: Kuf [M, N], the triangular solve and LowRankMultivariateNormal (the baseline)

    python tools/bench_gp_sgpr.py [--iters 5] [--min-n 0] [--max-n 1000000]

One VFE differentiable_loss + backward, RBF with ARD lengthscales, D = 8, f32, for N in {1e3, 1e4, 1e5, 1e6} and M in
{64, 256, 512}, and f64 at N = 1e5, M = 256.  (A float32 model runs the float64 kernels, M <= 256: at M = 512 both
columns are the dense route.)  Per route: milliseconds per step as the median of 5 blocks after one warm-up
block with the fastest and slowest block, and the allocator's peak above what the inputs hold (tools/bench_gp_kernel.py's
``blocks`` and ``peak_mib``).  The dense route is skipped where Kuf and autograd's copies of it do not fit.  The two
kernels alone (statistics forward, gradient backward) are timed by device events, with their fraction of the f32
matrix peak for 2 M^2 N flops each way.  One line of JSON per case."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import pyro_amd as pyro  # noqa: E402
import pyro_amd.contrib.gp as gp  # noqa: E402
from bench_gp_kernel import blocks, data, model_step, peak_mib  # noqa: E402
from pyro_amd import kernels  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3      # MI355X, v_mfma_f32_32x32x2_f32 (the data sheet's f32 matrix figure)


def events_ms(fn, iters, nblk=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(nblk):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) / iters)
    return statistics.median(ts), min(ts), max(ts)


def case(N, M, dtype, iters, dev, dense_limit_gib):
    X, y = data(N, 8, dtype, dev)
    pyro.clear_param_store()
    kern = gp.kernels.RBF(8, variance=torch.tensor(1.0, dtype=dtype), lengthscale=torch.ones(8, dtype=dtype)).to(dev)
    Xu = X[::max(N // M, 1)][:M].clone()
    model = gp.models.SparseGPRegression(X, y, kern, Xu, noise=torch.tensor(0.1, dtype=dtype, device=dev), approx="VFE",
                                         jitter=1e-4)
    step = model_step(model)
    out = {"case": "sgpr_vfe", "N": N, "M": Xu.size(0), "D": 8, "dtype": str(dtype).replace("torch.", "")}
    elem = 4 if dtype == torch.float32 else 8
    for route, fused in (("streamed", True), ("dense", False)):
        if not fused and 7.0 * M * N * elem / 2 ** 30 > dense_limit_gib:      # Kuf, W, autograd's copies: about 7 [M, N]
            out["dense_ms"] = "skipped: does not fit"
            continue
        gp.models.FUSED_SGPR, saved = fused, gp.models.FUSED_SGPR_MIN_N
        gp.models.FUSED_SGPR_MIN_N = 0
        try:
            out[route + "_ms"] = blocks(step, iters)
            out[route + "_peak_mib"] = peak_mib(step)
        except RuntimeError as e:                          # (the dense route's solve may fail to allocate at large N)
            out[route + "_ms"] = "does not run: " + str(e).splitlines()[0][:80]
            torch.cuda.empty_cache()
        finally:
            gp.models.FUSED_SGPR, gp.models.FUSED_SGPR_MIN_N = True, saved
    ls, var = torch.ones(8, dtype=dtype, device=dev), torch.ones(1, dtype=dtype, device=dev)
    r, gA, gb = y.reshape(-1, 1).contiguous(), torch.randn(M, M, dtype=dtype, device=dev), torch.randn(M, 1, dtype=dtype, device=dev)
    want = (False, True, True, True, False, False)
    flops = 2.0 * M * M * N
    for name, fn in (("fwd", lambda: kernels.gp_sgpr_fwd(X, Xu, r, ls, var)),
                     ("bwd", lambda: kernels.gp_sgpr_bwd(X, Xu, r, ls, var, None, gA, gb, "rbf", want))):
        med, lo, hi = events_ms(fn, iters)
        out["kernel_%s_ms" % name] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        if dtype == torch.float32:
            out["kernel_%s_fraction_of_f32_matrix_peak" % name] = round(flops / (med * 1e-3) / (F32_MATRIX_PEAK_TFLOPS * 1e12), 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=10 ** 6)
    ap.add_argument("--min-n", type=int, default=0)
    ap.add_argument("--dense-limit-gib", type=float, default=100.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for N in (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6):
        for M in (64, 256, 512):
            if args.min_n <= N <= args.max_n:
                case(N, M, torch.float32, args.iters, dev, args.dense_limit_gib)
    case(10 ** 5, 256, torch.float64, args.iters, dev, args.dense_limit_gib)


if __name__ == "__main__":
    main()
