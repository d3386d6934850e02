"""Generate tests/golden/mixture_rows.npz by running the UNMODIFIED reference (pyro-ppl/pyro 1.9.1 at /root/reference)
in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rows.py

The float64 loss and gradients of the reference's own TraceEnum_ELBO on two plated mixtures whose enumerated assignment
has per-row probabilities -- "experts" (``Categorical(logits=X @ W + b)``) and "grouped" (``Categorical(theta[g])``) of
tests/row_mixture_cases.py, N = 300, K = 3 --, with the tensors the models were built from.  The models have
parameters only (an empty guide): nothing is drawn.  `opt_einsum` (absent third-party dependency) is replaced by the
stand-in in oracle/refshim, as in make_golden.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))  # after `import torch` on purpose
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)                                     # (this project's `tests` package, not the reference's)

import pyro  # noqa: E402
import pyro.distributions as dist  # noqa: E402
import pyro.poutine as poutine  # noqa: E402
from pyro.infer import TraceEnum_ELBO  # noqa: E402

from tests.row_mixture_cases import make_row_mixture, row_init  # noqa: E402

assert pyro.__version__ == "1.9.1"


def main():
    flat = {}
    for form, seed in (("experts", 41), ("grouped", 42)):
        init = row_init("Normal", 300, 3, seed=seed)
        model, guide, x = make_row_mixture(form, init, torch.float64, "cpu", backend=(pyro, dist, poutine))
        pyro.clear_param_store()
        loss = TraceEnum_ELBO(max_plate_nesting=1).loss_and_grads(model, guide, x)
        flat[form + "/loss"] = np.asarray(loss)
        for k, v in init.items():
            flat[form + "/init/" + k] = v.numpy()
        for name, p in pyro.get_param_store().named_parameters():
            if p.grad is not None:
                flat[form + "/grad/" + name] = p.grad.detach().clone().numpy()
    path = os.path.join(HERE, "mixture_rows.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, {k: v.shape for k, v in flat.items()})


if __name__ == "__main__":
    main()
