"""The LinearHMM fixtures of tests/golden/linear_hmm.npz (made by tests/golden/make_golden_linear_hmm.py from the
unmodified reference, float64) as the host and device tests use them: loaded once, never modified."""
import os

import numpy as np
import torch

DRAW_CASES = ("h1_o1_t1", "h3_o2_b1_t2", "h3_o2_b3_t7_Fhet", "h3_o2_b3_t7_Hhet", "h8_o8_b2_t6", "h5_o12_b2_t4",
              "h16_o16_b2_t5", "h3_o2_b2_t5_exp")
# name: (the reparameterised components, IndependentHMM, exp transform)
REP_CASES = {"trans_obs": (("trans", "obs"), False, False), "init_trans_obs": (("init", "trans", "obs"), False, False),
             "independent": (("trans", "obs"), True, False), "exp": (("trans", "obs"), False, True)}
PARAMS = ("F", "H", "init_loc", "init_scale", "trans_df", "trans_loc", "trans_scale", "obs_df", "obs_loc",
          "obs_scale")
NOISE = ("init", "e", "n")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_hmm.npz")
_CACHE = {}


def golden(kind, case):
    """{name: numpy array} of one case of ``kind`` "draw" or "rep"."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                k, c, name = key.split("/")
                _CACHE.setdefault((k, c), {})[name] = z[key]
        for c in _CACHE.values():
            for a in c.values():
                a.setflags(write=False)
    return _CACHE[(kind, case)]


def tensors(g, names, dtype, device, requires_grad=False):
    return {k: torch.tensor(g[k], dtype=dtype, device=device, requires_grad=requires_grad) for k in names if k in g}


def build(t, dist, T, exp=False, normal=None):
    """The LinearHMM of a case from the tensors ``t`` with the distribution classes of module ``dist``; ``normal``:
    the Normal class to use (the package's own draws on the device alone; the host tests pass torch's)."""
    if "init_df" in t:
        init = dist.Independent(dist.StudentT(t["init_df"], t["init_loc"], t["init_scale"]), 1)
    else:
        init = dist.Independent((normal or dist.Normal)(t["init_loc"], t["init_scale"]), 1)
    trans = dist.Independent(dist.StudentT(t["trans_df"], t["trans_loc"], t["trans_scale"]), 1)
    obs = dist.Independent(dist.StudentT(t["obs_df"], t["obs_loc"], t["obs_scale"]), 1)
    if exp:
        obs = dist.TransformedDistribution(obs, [torch.distributions.transforms.ExpTransform()])
    return dist.LinearHMM(init, t["F"], trans, t["H"], obs, duration=T)


def loop(F, H, init, e, n):
    """z_t = z_{t-1} F_t + e_t, y_t = z_t H_t + n_t in torch ops: F [B | 1, T | 1, h, h], H [B | 1, T | 1, h, o],
    the noise [S, B, ...] -> (y [S, B, T, o], z [S, B, T, h]), in the dtype and on the device of its inputs."""
    z, ys, zs = init, [], []
    for t in range(e.shape[-2]):
        Ft = F[:, t if F.shape[1] > 1 else 0]
        Ht = H[:, t if H.shape[1] > 1 else 0]
        z = (z.unsqueeze(-2) @ Ft).squeeze(-2) + e[..., t, :]
        zs.append(z)
        ys.append((z.unsqueeze(-2) @ Ht).squeeze(-2) + n[..., t, :])
    return torch.stack(ys, dim=-2), torch.stack(zs, dim=-2)
