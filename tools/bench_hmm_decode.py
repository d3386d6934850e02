"""Reading a decoding out of a fitted HMM (developer tool): infer_discrete on examples/hmm.py model_1's shapes
(229 sequences x 129 steps x 16 states, 88 tones, f32) at temperature 0 (the Viterbi paths) and 1 (one joint posterior
draw), by the chain kernel (csrc/logchain_decode.hip: one launch for all 129 sites) and with
``contract.FUSED_CHAIN = False`` in the same tree (the generic route: one contraction of the whole chain per site).

    python tools/bench_hmm_decode.py [--shape S:L:K:D] [--no-launches]

Per temperature and route: milliseconds per call as the median of 5 blocks after one warm-up call (one call per block
on the generic route, three on the kernel's), with the fastest and slowest block; each block ends with a device
synchronisation, so a number covers the host work, every launch and the device time of one call.  Launches per call:
device activities of one call seen by torch.profiler.  The two routes' values are compared site by site (they use the
same uniforms; float32 ties and near-ties may differ).  Validation is off."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pyro_amd as pyro  # noqa: E402
from pyro_amd import examples, poutine  # noqa: E402
from pyro_amd.infer import infer_discrete  # noqa: E402
from pyro_amd.ops import contract  # noqa: E402


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


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def route(fused, fn):
    def call():
        contract.FUSED_CHAIN = fused
        try:
            return fn()
        finally:
            contract.FUSED_CHAIN = True
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="229:129:16:88")
    ap.add_argument("--no-launches", action="store_true")
    args = ap.parse_args()
    S, L, K, D = (int(v) for v in args.shape.split(":"))
    dev = torch.device("cuda:0")
    seqs, lengths = examples.synthetic_hmm_data(S, L, D, dev)
    pyro.clear_param_store()
    pyro.set_rng_seed(0)
    pyro.enable_validation(False)
    model = lambda: examples.hmm_model_1(seqs, lengths, K)      # noqa: E731
    with torch.no_grad():
        model()                                                  # the parameters exist from here on

    def states(decoded):
        tr = poutine.trace(decoded).get_trace()
        return torch.stack([tr.nodes["x_{}".format(t)]["value"].reshape(-1) for t in range(L)], -1)

    for temperature in (0, 1):
        decoded = infer_discrete(model, first_available_dim=-3, temperature=temperature)
        out = {"shape": [S, L, K, D], "temperature": temperature}
        values = {}
        for name, fused in (("kernel", True), ("generic", False)):
            def one():
                with torch.no_grad():
                    return decoded()
            call = route(fused, one)
            med, lo, hi = blocks(call, 3 if fused else 1)
            out[name + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
            if not args.no_launches:
                try:
                    out[name + "_launches"] = launches_of(call)
                except Exception as e:                           # noqa: BLE001  (the profiler is optional)
                    out[name + "_launches"] = "not counted: %s" % type(e).__name__
            pyro.set_rng_seed(1)
            values[name] = route(fused, lambda: states(decoded))()
        out["same_states"] = round(float((values["kernel"] == values["generic"]).double().mean()), 6)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
