"""Generate tests/golden/gp_wrap.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_gp_wrap.py

The reference is imported as tests/golden/make_golden_gp.py imports it.  The table is the tests' own
(tests/gp_wrap_cases.py, on the data of tests/gp_cases.py), run here on the reference.

weights/{W, c, v}          the input warping x W + c and the vector of the vertical scaling 1 + tanh(x v) / 2
kern/<id>/{K, KZ, diag}    K(X), K(X, Xnew) and the diagonal of Cosine, Brownian, Exponent, Warping, VerticalScaling and
                           their nestings
kern/<id>/g*               the gradients of sum(K G) + sum(KZ H) for fixed G, H: gX, gZ, g_<parameter>, g_<weight>
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


def _cases(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gc, wc = _cases("gp_cases"), _cases("gp_wrap_cases")

assert pyro.__version__ == "1.9.1"
torch.set_default_dtype(torch.float64)


def main():
    data, w = gc.fixture_data(), wc.weights()
    flat = {"weights/" + n: v.detach().numpy() for n, v in w.items()}
    for kid, kern in wc.kernel_table(gp, w).items():
        pyro.clear_param_store()
        for name, value in wc.record(kern, data["X"], data["Xnew"], w).items():
            flat["kern/%s/%s" % (kid, name)] = value
    np.savez_compressed(wc.GOLDEN, **flat)
    print("wrote", wc.GOLDEN, os.path.getsize(wc.GOLDEN), "bytes,", len(flat), "arrays")


if __name__ == "__main__":
    main()
