"""Generate tests/golden/gp.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_gp.py

The reference is imported as tests/golden/make_golden_time_transforms.py imports it (oracle/refshim stands in for
opt_einsum).  The tables of kernels, models and inputs are the tests' own (tests/gp_cases.py), run here on the
reference; only the data file depends on it.

kern/<id>/{K, KZ, diag}        K(X), K(X, Xnew) and the diagonal of every kernel of gp_cases.kernel_table
cond/<scale><whiten><full>/    loc and cov of util.conditional for each combination, and p_loc, p_cov from inputs
                               perturbed by 1e-13 relative
model/<name>/<variant>/        variant "plain" or "prior" (LogNormal prior on the lengthscale, its latent fixed):
                               loss, grad_<parameter>, and the same from y perturbed by 1e-13 relative (p_loss, p_grad_*)
model/<name>/forward/<c><n>/   loc, cov of forward(Xnew, full_cov=c, noiseless=n), and p_loc, p_cov (y, X and Xnew perturbed)
model/<name>/train             the losses of ten util.train steps with torch.optim.Adam(lr=0.01), and p_train
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))  # after `import torch` on purpose
sys.path.insert(0, os.environ.get("PYRO_REFERENCE", "/root/reference"))

import pyro  # noqa: E402
import pyro.contrib.gp as gp  # noqa: E402
import pyro.distributions as dist  # noqa: E402
from pyro.infer import Trace_ELBO  # noqa: E402
from pyro.nn import PyroSample  # noqa: E402


def _cases(name):
    """A case module of this repository's tests by its path (the reference has a ``tests`` package of its own)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gc = _cases("gp_cases")

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)


def kernels(flat, data):
    for kid, kern in gc.kernel_table(gp).items():
        pyro.clear_param_store()      # (unnamed top-level modules share the store's names: "variance", "lengthscale")
        with torch.no_grad():
            flat["kern/%s/K" % kid] = kern(data["X"]).numpy()
            flat["kern/%s/KZ" % kid] = kern(data["X"], data["Xnew"]).numpy()
            flat["kern/%s/diag" % kid] = kern(data["X"], diag=True).numpy()


def conditionals(flat, data):
    kern = gc.kernel_table(gp)["matern52_ard"]
    pyro.clear_param_store()
    for scale, whiten, full in gc.CONDITIONAL_CASES:
        with torch.no_grad():
            loc, cov = gp.util.conditional(data["Xnew"], data["X"], kern, data["f_loc"],
                                           data["f_scale_tril"] if scale else None, full_cov=full, whiten=whiten)
        key = "cond/%d%d%d/" % (scale, whiten, full)
        flat[key + "loc"], flat[key + "cov"] = loc.numpy(), cov.numpy()
        wiggle = gc.perturbed_inputs(data)
        with torch.no_grad():
            loc, cov = gp.util.conditional(wiggle["Xnew"], wiggle["X"], kern, wiggle["f_loc"],
                                           wiggle["f_scale_tril"] if scale else None, full_cov=full, whiten=whiten)
        flat[key + "p_loc"], flat[key + "p_cov"] = loc.numpy(), cov.numpy()


def models(flat, data):
    for name in gc.MODELS:
        for tag, y in (("", None), ("p_", gc.perturbed_y(data))):
            for variant, prior in (("plain", None), ("prior", (PyroSample, dist))):
                pyro.clear_param_store()
                model = gc.build_model(gp, name, data, prior=prior, y=y)
                loss, grads = gc.loss_and_grads(model, Trace_ELBO())
                key = "model/%s/%s/" % (name, variant)
                flat[key + tag + "loss"] = np.array(loss)
                for pname, g in grads.items():
                    flat[key + tag + "grad_" + pname] = g
                print(name, variant, tag, loss, sorted(grads))
            pyro.clear_param_store()
            # (the predictive covariance does not depend on y: the perturbed forward perturbs X and Xnew as well)
            inputs = data if y is None else dict(data, **{k: gc.perturbed_inputs(data)[k] for k in ("X", "Xnew")})
            model = gc.build_model(gp, name, inputs, y=y)
            for full, noiseless in gc.FORWARD_CASES:
                with torch.no_grad():
                    loc, cov = model(inputs["Xnew"], full_cov=full, noiseless=noiseless)
                key = "model/%s/forward/%d%d/" % (name, full, noiseless)
                flat[key + tag + "loc"], flat[key + tag + "cov"] = loc.numpy(), cov.numpy()
            pyro.clear_param_store()
            model = gc.build_model(gp, name, data, y=y)
            losses = gp.util.train(model, torch.optim.Adam(model.parameters(), lr=0.01), num_steps=gc.TRAIN_STEPS)
            flat["model/%s/%strain" % (name, tag)] = np.array(losses)


def main():
    flat = {}
    data = gc.fixture_data()
    kernels(flat, data)
    conditionals(flat, data)
    models(flat, data)
    path = os.path.join(HERE, "gp.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes,", len(flat), "arrays")


if __name__ == "__main__":
    main()
