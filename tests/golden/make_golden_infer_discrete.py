"""Generate tests/golden/infer_discrete.npz by running the UNMODIFIED reference (pyro-ppl/pyro 1.9.1; its checkout
is named by the environment variable PYRO_REFERENCE) in the build container:

    PYRO_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_infer_discrete.py

The reference's own ``infer_discrete(..., temperature=0)`` in float64 on two models of tests/assign_cases.py, with the
tensors the models were built from: a plated Gaussian mixture (N = 40, K = 3) and a ``pyro.markov`` chain (5 steps,
3 states).  Nothing is drawn.  `opt_einsum` (absent third-party dependency) is replaced by the stand-in in
oracle/refshim, as in make_golden.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))  # after `import torch` on purpose
sys.path.insert(0, os.environ["PYRO_REFERENCE"])
sys.path.insert(0, ROOT)                                     # (this project's `tests` package, not the reference's)

import pyro  # noqa: E402
import pyro.distributions as dist  # noqa: E402
from pyro.infer import infer_discrete  # noqa: E402

from tests import assign_cases as ac  # noqa: E402

assert pyro.__version__ == "1.9.1"


def main():
    flat = {}
    T = ac.gmm_tensors(40, 3, seed=31)
    z = infer_discrete(ac.make_gmm(T, backend=(pyro, dist)), first_available_dim=-2, temperature=0)()
    for k, v in T.items():
        flat["gmm/" + k] = v.numpy()
    flat["gmm/z"] = z.numpy()
    H = ac.hmm_tensors(5, 3, seed=0)
    xs = infer_discrete(ac.make_hmm(H, backend=(pyro, dist)), first_available_dim=-1, temperature=0)()
    for k, v in H.items():
        flat["hmm/" + k] = v.numpy()
    flat["hmm/xs"] = torch.stack([x.reshape(()) for x in xs]).numpy()
    path = os.path.join(HERE, "infer_discrete.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, {k: v.shape for k, v in flat.items()})
    print(flat["gmm/z"], flat["hmm/xs"])


if __name__ == "__main__":
    main()
