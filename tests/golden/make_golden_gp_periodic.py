"""Generate tests/golden/gp_periodic.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_gp_periodic.py

The reference is imported as tests/golden/make_golden_gp.py imports it.  The tables are the tests' own
(tests/gp_periodic_cases.py, on the data of tests/gp_cases.py), run here on the reference.

kern/<id>/{K, KZ, diag}   K(X), K(X, Xnew) and the diagonal of Periodic (scalar, ARD, active_dims) and Product(Periodic, RBF)
model/                    GPRegression over Product(Periodic, RBF): loss, grad_<parameter>, and the same from y
                          perturbed by 1e-13 relative (p_loss, p_grad_*)
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
from pyro.infer import Trace_ELBO  # noqa: E402


def _cases(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gc, pc = _cases("gp_cases"), _cases("gp_periodic_cases")

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)


def main():
    flat = {}
    data = gc.fixture_data()
    for kid, kern in pc.kernel_table(gp).items():
        pyro.clear_param_store()
        with torch.no_grad():
            flat["kern/%s/K" % kid] = kern(data["X"]).numpy()
            flat["kern/%s/KZ" % kid] = kern(data["X"], data["Xnew"]).numpy()
            flat["kern/%s/diag" % kid] = kern(data["X"], diag=True).numpy()
    for tag, y in (("", None), ("p_", gc.perturbed_y(data))):
        pyro.clear_param_store()
        loss, grads = gc.loss_and_grads(pc.build_model(gp, data, y=y), Trace_ELBO())
        flat["model/" + tag + "loss"] = np.array(loss)
        for pname, g in grads.items():
            flat["model/" + tag + "grad_" + pname] = g
        print(tag, loss, sorted(grads))
    np.savez_compressed(pc.GOLDEN, **flat)
    print("wrote", pc.GOLDEN, os.path.getsize(pc.GOLDEN), "bytes,", len(flat), "arrays")


if __name__ == "__main__":
    main()
