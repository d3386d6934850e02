"""Generate tests/golden/gaussian_hmm_edges.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1): for every
layout case of tests/gaussian_hmm_edge_cases.py at the narrow width (hidden 3, obs 2, B = 3, T = 5) the inputs of a
GaussianHMM, its log_prob, the autograd gradients of sum(log_prob) with respect to every input and the moments of
filter(), all float64 on the CPU -- what tests/golden/make_golden_gaussian_hmm.py stores for its cases.

    python tests/golden/make_golden_gaussian_hmm_edges.py

The reference is imported as make_golden_gaussian_hmm.py imports it; the inputs come from the case generators of
tests/gaussian_hmm_edge_cases.py (seeded numpy), so that running this again reproduces the file.  In these cases every
leaf carries its batch and step axes explicitly, of size 1 where the parameter is shared or time-homogeneous: the
reference broadcasts them.  Only the data file depends on the reference; the tests read nothing else of it.
"""
import os
import sys

import numpy as np
import torch

from make_golden_gaussian_hmm import HERE, NAMES, ROOT, build  # (puts the reference on the path and imports it)

sys.path.insert(0, ROOT)
from tests import gaussian_hmm_edge_cases as ec  # noqa: E402


def main():
    flat = {}
    h, o = ec.A_WIDTHS[0]
    for lay in ec.LAYOUTS:
        arrays = ec.inputs(("A", lay, h, o))
        B, T = arrays["x"].shape[:2]
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in arrays.items()}
        hmm = build(t, "mvn")
        assert hmm.batch_shape == (B,), (lay, hmm.batch_shape)
        lp = hmm.log_prob(t["x"])
        grads = torch.autograd.grad(lp.sum(), [t[k] for k in NAMES])
        with torch.no_grad():
            post = build({k: v.detach() for k, v in t.items()}, "mvn").filter(t["x"].detach())
            fm = post.loc.expand(B, h)
            fP = post.covariance_matrix.expand(B, h, h)
        for k in NAMES:
            flat[lay + "/" + k] = arrays[k]
        for k, g in zip(NAMES, grads):
            flat[lay + "/g_" + k] = g.numpy()
        flat[lay + "/log_prob"] = lp.detach().numpy()
        flat[lay + "/filter_mean"] = fm.numpy()
        flat[lay + "/filter_cov"] = fP.numpy()
        print(lay, "log_prob", lp.detach().numpy())
    path = os.path.join(HERE, "gaussian_hmm_edges.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
