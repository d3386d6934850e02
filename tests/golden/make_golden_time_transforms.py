"""Generate tests/golden/time_transforms.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_time_transforms.py

The reference is imported as tests/golden/make_golden_forecast.py imports it (oracle/refshim stands in for
opt_einsum).  The cases, inputs and the model text are the tests' own (tests/time_transform_cases.py, which reads
tests/forecast_cases.py and the inputs of tests/golden/forecast.npz), run here on the reference; only the data file
depends on it.

ops/<case>/<op>             dct, idct, haar_transform, inverse_haar_transform along dim -2 of the fixture-shaped cases
transforms/<case>/          y = T(x), inv = T.inv(x), ladj = T.log_abs_det_jacobian(x, y) of the transform classes
periodic/<helper>_<k>       periodic_repeat, periodic_cumsum and periodic_features on three inputs each
traces/<noise>/<reparam>/<config>/   sites, log_prob_<site> and value_drift of the drift model under poutine.reparam
                            with an explicit config function, the global latents and the auxiliary site conditioned
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))  # after `import torch` on purpose
sys.path.insert(0, os.environ.get("PYRO_REFERENCE", "/root/reference"))

import pyro  # noqa: E402
import pyro.distributions as dist  # noqa: E402
from pyro import poutine  # noqa: E402
from pyro.contrib.forecast import ForecastingModel  # noqa: E402
from pyro.distributions import transforms  # noqa: E402
from pyro.infer.reparam import DiscreteCosineReparam, HaarReparam  # noqa: E402
from pyro.ops import tensor_utils  # noqa: E402


def _cases(name):
    """A case module of this repository's tests by its path (the reference has a ``tests`` package of its own)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


ttc = _cases("time_transform_cases")
fc = ttc.fc

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)
NS = types.SimpleNamespace(pyro=pyro, dist=dist, poutine=poutine, ForecastingModel=ForecastingModel,
                           HaarReparam=HaarReparam, DiscreteCosineReparam=DiscreteCosineReparam)


def ops(flat):
    for case in ttc.CASES:
        if case[0] > max(ttc.SMALL_N) or case[1:3] != ttc.FIXTURE_SHAPE:
            continue
        x = ttc.make(case)
        for op in ttc.OPS:
            flat["ops/%s/%s" % (ttc.case_id(case), op)] = ttc.along_time(getattr(tensor_utils, op), x).numpy()


def transform_classes(flat):
    x = ttc.transform_input()
    for case in ttc.TRANSFORM_CASES:
        t = ttc.build_transform(transforms, case)
        key = "transforms/%s/" % ttc.transform_id(case)
        y = t(x)
        flat[key + "y"], flat[key + "inv"] = y.numpy(), t.inv(x).numpy()
        flat[key + "ladj"] = t.log_abs_det_jacobian(x, y).numpy()


def periodic(flat):
    inputs = ttc.periodic_inputs()
    for k, args in enumerate(inputs["repeat"]):
        flat["periodic/repeat_%d" % k] = tensor_utils.periodic_repeat(*args).numpy()
    for k, args in enumerate(inputs["cumsum"]):
        flat["periodic/cumsum_%d" % k] = tensor_utils.periodic_cumsum(*args).numpy()
    for k, args in enumerate(inputs["features"]):
        flat["periodic/features_%d" % k] = tensor_utils.periodic_features(*args, dtype=torch.float64).numpy()


def traces(flat):
    t = fc.tensors(fc.golden("inputs"))
    coef = ttc.drift_coefficients()
    for noise in ttc.DRIFT_NOISES:
        for which in ttc.REPARAMS:
            for config, particles, nesting in fc.CONFIGS:
                tr = ttc.run_reparam_trace(NS, noise, which, t, particles, nesting, coef)
                sites = fc.sample_sites(tr)
                key = ttc.trace_key(noise, which, config) + "/"
                flat[key + "sites"] = np.array(sites)
                for s in sites:
                    flat[key + "log_prob_" + s] = tr.nodes[s]["log_prob"].detach().numpy()
                flat[key + "value_drift"] = tr.nodes["drift"]["value"].detach().numpy()
                print(noise, which, config, sites, float(tr.log_prob_sum()))


def main():
    flat = {}
    ops(flat)
    transform_classes(flat)
    periodic(flat)
    traces(flat)
    path = os.path.join(HERE, "time_transforms.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
