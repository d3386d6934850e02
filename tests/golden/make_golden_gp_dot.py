"""Generate tests/golden/gp_dot.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_gp_dot.py

The reference is imported as tests/golden/make_golden_gp.py imports it; the tables are tests/gp_dot_cases.py's.
kern/<id>/{K, KZ, diag, gX, gZ, g_<parameter>}   gp_dot_cases.record of every kernel of its table
model/{loss, p_loss}                             its model's loss, and the same from y perturbed by 1e-13 relative
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


gc, dc = _cases("gp_cases"), _cases("gp_dot_cases")

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)


def main():
    flat = {}
    data = gc.fixture_data()
    for kid, kern in dc.kernel_table(gp).items():
        pyro.clear_param_store()
        for name, value in dc.record(kern, data["X"], data["Xnew"]).items():
            flat["kern/%s/%s" % (kid, name)] = value
    for tag, y in (("", None), ("p_", gc.perturbed_y(data))):
        pyro.clear_param_store()
        loss, _ = gc.loss_and_grads(dc.build_model(gp, data, y=y), Trace_ELBO())
        flat["model/" + tag + "loss"] = np.array(loss)
    np.savez_compressed(dc.GOLDEN, **flat)
    print("wrote", dc.GOLDEN, os.path.getsize(dc.GOLDEN), "bytes,", len(flat), "arrays")


if __name__ == "__main__":
    main()
