"""Generate tests/golden/adam_edges.npz from the UNMODIFIED reference's ClippedAdam (pyro-ppl/pyro 1.9.1,
pyro/optim/clipped_adam.py), float64 on the CPU.

    python tests/golden/make_golden_adam_edges.py

The reference is imported as tests/golden/make_golden_time_transforms.py imports it (oracle/refshim stands in for
opt_einsum).  The cases are the tests' own (tests/guide_edge_cases.py); only the data file depends on the reference.

pool/{p,g,m,v}          the 61-element input pool every case reads (float32-representable float64)
C/h<h>_s<step0>/        one step of hyper-parameter set h of guide_edge_cases.adam_hypers(True) from the pool's
                        state with ``state["step"]`` preset to step0 and ``group["lr"]`` to lr * lrd**step0:
                        hy = [lr, beta1, beta2, eps, weight_decay, clip_norm, lrd, step0], and p, m, v afterwards
C/v_<variant>/          the same for the edge gradients (default set, step0 = 1) and for lr = 0 with weight decay
C/traj/{p,m,v}          [5, 61]: after each of five steps from zero moments (ADAM_TRAJ_HYPER, adam_traj_grad)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from tests import guide_edge_cases as gc  # noqa: E402  (before the reference's own ``tests`` package is reachable)

sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, os.environ.get("PYRO_REFERENCE", "/root/reference"))

import pyro  # noqa: E402
from pyro.optim.clipped_adam import ClippedAdam  # noqa: E402

assert pyro.__version__ == "1.9.1"


def optimizer(p, hy, step0, m=None, v=None):
    P = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = ClippedAdam([P], lr=hy["lr"] * hy["lrd"] ** step0, betas=hy["betas"], eps=hy["eps"],
                      weight_decay=hy["wd"], clip_norm=hy["clip"], lrd=hy["lrd"])
    if m is not None:
        opt.state[P] = {"step": step0, "exp_avg": torch.tensor(m, dtype=torch.float64),
                        "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
    return P, opt


def one_step(flat, key, pool, hy, step0, variant=None):
    p, g, m, v = gc.adam_inputs(pool, hy, gc.ADAM_POOL, variant)
    P, opt = optimizer(p, hy, step0, m, v)
    P.grad = torch.tensor(g, dtype=torch.float64)
    opt.step()
    st = opt.state[P]
    assert st["step"] == step0 + 1
    flat[key + "/hy"] = np.array([hy["lr"], *hy["betas"], hy["eps"], hy["wd"], hy["clip"], hy["lrd"], step0])
    flat[key + "/p"], flat[key + "/m"], flat[key + "/v"] = (x.detach().numpy().copy() for x in
                                                            (P, st["exp_avg"], st["exp_avg_sq"]))


def main():
    pool = gc.make_adam_pool()
    flat = {"pool/" + k: x for k, x in pool.items()}
    hypers = gc.adam_hypers(True)
    for h, step0 in gc.adam_single_keys(True):
        one_step(flat, gc.adam_golden_key(h, step0), pool, hypers[h], step0)
    for variant in ("zero", "zero_state", "naninf", "big"):
        one_step(flat, gc.adam_golden_key(0, 1, variant), pool, hypers[0], 1, variant)
    one_step(flat, gc.adam_golden_key(0, 1, "lr0wd"), pool, gc.ADAM_LR0WD_HYPER, 1)
    P, opt = optimizer(pool["p"], gc.ADAM_TRAJ_HYPER, 0)
    traj = {w: [] for w in "pmv"}
    for s in range(gc.ADAM_TRAJ_STEPS):
        P.grad = torch.tensor(gc.adam_traj_grad(pool, s), dtype=torch.float64)
        opt.step()
        st = opt.state[P]
        for w, x in zip("pmv", (P, st["exp_avg"], st["exp_avg_sq"])):
            traj[w].append(x.detach().numpy().copy())
    for w in "pmv":
        flat["C/traj/" + w] = np.stack(traj[w])
    path = os.path.join(HERE, "adam_edges.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes;", len(flat), "arrays")


if __name__ == "__main__":
    main()
