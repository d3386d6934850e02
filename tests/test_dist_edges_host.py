"""The numpy oracle (oracle/dists.py), which the GPU tests trust, against float64 torch on the edge
grids of tests/dist_edge_cases.py: overflow, underflow, support boundaries, NaN / inf operands.
The float64 rule of that module applies."""
import numpy as np
import pytest
import torch

from oracle import dists as o_dists
from tests import dist_edge_cases as ec


@pytest.mark.parametrize("f32_grid", [False, True], ids=["grid64", "grid32"])
@pytest.mark.parametrize("dist_id", sorted(ec.NAMES))
def test_oracle_log_prob_and_grad_match_torch_at_the_edges(dist_id, f32_grid):
    v, a, b = ec.grid(dist_id, f32_grid)
    ref = ec.reference(dist_id, v, a, b, torch.float64)
    M = ec.magnitude(dist_id, v, a, b)
    bb = b if dist_id in ec.TWO_PARAM else None
    with np.errstate(all="ignore"):
        lp = np.broadcast_to(o_dists.LOG_PROB[dist_id](v, a, bb), v.shape)
        grads = o_dists.log_prob_grad(dist_id, v, a, bb)
    name = ec.NAMES[dist_id]
    ec.check(name + " log_prob", lp, ref["lp"], M["lp"], False, inputs=(v, a, b),
             nan_ok=ec.kept_nan(dist_id, "lp", v, a, b))
    for k, g in zip(("dv", "da", "db"), grads):
        if k == "db" and dist_id not in ec.TWO_PARAM:
            continue
        ec.check("%s %s" % (name, k), np.broadcast_to(g, v.shape), ref[k], M[k], False, inputs=(v, a, b))


def test_oracle_kl_pieces_sum_to_minus_torch_kl():
    lq, sq, lp, sp = ec._prod([0.0, 3.0, -1e6], [1e-30, 1.0, 1e6], [0.5, -2e6], [1e-6, 1.0, 1e30])
    with np.errstate(all="ignore"):
        got = o_dists.kl_normal_loc_half(lq, lp, sp) + o_dists.kl_normal_scale_half(sq, sp)
    ref = -torch.distributions.kl_divergence(torch.distributions.Normal(torch.tensor(lq), torch.tensor(sq)),
                                             torch.distributions.Normal(torch.tensor(lp), torch.tensor(sp)))
    M = ec.magnitude(10, lq, lp, sp)["lp"] + ec.magnitude(11, sq, sp, sp)["lp"]
    ec.check("KL pieces", got, ref.numpy(), M, False, inputs=(lq, sq, lp, sp))
