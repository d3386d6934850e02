"""Generate tests/golden/linear_hmm.npz from the UNMODIFIED reference (pyro-ppl/pyro 1.9.1), float64 on the CPU.

    python tests/golden/make_golden_linear_hmm.py

The reference is imported as tests/golden/make_golden_gaussian_hmm.py imports it (oracle/refshim stands in for
opt_einsum).  Only the data file depends on the reference; the tests read nothing else of it.

Draw cases ("draw/<case>/..."): the matrices F, H, the components' parameters, the noise triple (init, e, n) and the
reference's LinearHMM.rsample((3,)) output x.  The noise is captured by seeding torch, drawing the three components'
rsample in the order LinearHMM.rsample does, reseeding with the same seed and calling hmm.rsample; the generator
recomputes x from the stored noise with a plain loop and asserts agreement at 1e-13, so a fixture whose noise is not
the noise used cannot be written.

Reparameterisation cases ("rep/<case>/..."): the parameters, the data, the values the reference drew for every
auxiliary Gamma site and the log_prob of every site of
poutine.trace(poutine.reparam(model, config={"hmm": LinearHMMReparam(...)})).

Noise families: Normal initial, StudentT transition and observation with df between 2 and 5.  F is scaled to spectral
norm 0.9.
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
import pyro.distributions as dist  # noqa: E402
from pyro import poutine  # noqa: E402
from pyro.infer.reparam import LinearHMMReparam, StudentTReparam  # noqa: E402

assert pyro.__version__ == "1.9.1"

S = 3
# name: (B, T, hidden, obs, F layout, H layout, exp transform); a layout is (per-series, per-step)
DRAW_CASES = {
    "h1_o1_t1": (2, 1, 1, 1, (True, True), (True, True), False),
    "h3_o2_b1_t2": (1, 2, 3, 2, (True, True), (True, True), False),
    "h3_o2_b3_t7_Fhet": (3, 7, 3, 2, (True, True), (False, False), False),
    "h3_o2_b3_t7_Hhet": (3, 7, 3, 2, (False, False), (True, True), False),
    "h8_o8_b2_t6": (2, 6, 8, 8, (True, False), (False, True), False),
    "h5_o12_b2_t4": (2, 4, 5, 12, (False, True), (True, False), False),
    "h16_o16_b2_t5": (2, 5, 16, 16, (True, True), (True, True), False),
    "h3_o2_b2_t5_exp": (2, 5, 3, 2, (False, False), (False, False), True),
}
PARAMS = ("F", "H", "init_loc", "init_scale", "trans_df", "trans_loc", "trans_scale", "obs_df", "obs_loc",
          "obs_scale")
# name: (B, T, hidden, obs, which components are reparameterised, IndependentHMM, exp transform)
REP_CASES = {
    "trans_obs": (2, 6, 3, 2, ("trans", "obs"), False, False),
    "init_trans_obs": (2, 5, 3, 2, ("init", "trans", "obs"), False, False),
    "independent": (2, 5, 2, 3, ("trans", "obs"), True, False),
    "exp": (2, 5, 3, 2, ("trans", "obs"), False, True),
}


def make_params(rng, lead, T, h, o, f_lay, h_lay, student_init=False):
    """``lead``: the batch shape.  Matrices per layout; component parameters per series, time-homogeneous (the class
    expands them)."""
    def mat(lay, rows, cols):
        shape = (lead if lay[0] else (1,) * len(lead)) + ((T,) if lay[1] else (1,)) + (rows, cols)
        return rng.standard_normal(shape)

    F = mat(f_lay, h, h)
    F = F * (0.9 / np.linalg.norm(F, ord=2, axis=(-2, -1)))[..., None, None]
    p = {"F": F, "H": mat(h_lay, h, o) / np.sqrt(h),
         "init_loc": 0.3 * rng.standard_normal(lead + (h,)), "init_scale": 0.5 + rng.random(lead + (h,)),
         "trans_df": 2.0 + 3.0 * rng.random(lead + (1, h)), "trans_loc": 0.3 * rng.standard_normal(lead + (1, h)),
         "trans_scale": 0.5 + rng.random(lead + (1, h)),
         "obs_df": 2.0 + 3.0 * rng.random(lead + (1, o)), "obs_loc": 0.3 * rng.standard_normal(lead + (1, o)),
         "obs_scale": 0.5 + rng.random(lead + (1, o))}
    if student_init:
        p["init_df"] = 2.0 + 3.0 * rng.random(lead + (h,))
    return p


def build(t, exp=False):
    if "init_df" in t:
        init = dist.StudentT(t["init_df"], t["init_loc"], t["init_scale"]).to_event(1)
    else:
        init = dist.Normal(t["init_loc"], t["init_scale"]).to_event(1)
    trans = dist.StudentT(t["trans_df"], t["trans_loc"], t["trans_scale"]).to_event(1)
    obs = dist.StudentT(t["obs_df"], t["obs_loc"], t["obs_scale"]).to_event(1)
    if exp:
        obs = dist.TransformedDistribution(obs, dist.transforms.ExpTransform())
    T = max(t["F"].shape[-3], t["H"].shape[-3])
    return dist.LinearHMM(init, t["F"], trans, t["H"], obs, duration=T if T > 1 else t["_T"])


def plain_loop(F, H, init, e, n, exp):
    T = e.shape[-2]
    z, ys = init, []
    for t in range(T):
        Ft = F[..., t if F.shape[-3] > 1 else 0, :, :]
        Ht = H[..., t if H.shape[-3] > 1 else 0, :, :]
        z = np.einsum("...i,...ij->...j", z, Ft) + e[..., t, :]
        ys.append(np.einsum("...i,...ij->...j", z, Ht) + n[..., t, :])
    y = np.stack(ys, axis=-2)
    return np.exp(y) if exp else y


def draw_cases(rng, flat):
    for k, (name, (B, T, h, o, f_lay, h_lay, exp)) in enumerate(DRAW_CASES.items()):
        arrays = make_params(rng, (B,), T, h, o, f_lay, h_lay)
        t = {key: torch.tensor(v, dtype=torch.float64) for key, v in arrays.items()}
        t["_T"] = T
        hmm = build(t, exp)
        assert hmm.batch_shape == (B,) and hmm.event_shape == (T, o) and hmm.duration == T, name
        seed = 1000 + k
        torch.manual_seed(seed)
        init = hmm.initial_dist.rsample((S,))
        e = hmm.transition_dist.expand(hmm.batch_shape + (T,)).rsample((S,))
        n = hmm.observation_dist.expand(hmm.batch_shape + (T,)).rsample((S,))
        torch.manual_seed(seed)
        x = hmm.rsample((S,))
        assert x.shape == (S, B, T, o)
        again = plain_loop(arrays["F"], arrays["H"], init.numpy(), e.numpy(), n.numpy(), exp)
        err = np.max(np.abs(again - x.numpy())) / (1.0 + np.max(np.abs(x.numpy())))
        print("draw", name, "plain loop against the reference %.1e" % err)
        assert err <= 1e-13, (name, err)
        for key in PARAMS:
            flat["draw/%s/%s" % (name, key)] = arrays[key]
        for key, v in (("init", init), ("e", e), ("n", n), ("x", x)):
            flat["draw/%s/%s" % (name, key)] = v.numpy()


def rep_cases(rng, flat):
    for k, (name, (B, T, h, o, parts, indep, exp)) in enumerate(REP_CASES.items()):
        lead = (B, o) if indep else (B,)
        arrays = make_params(rng, lead, T, h, 1 if indep else o, (False, False), (False, False),
                             student_init="init" in parts)
        x = rng.standard_normal((B, T, o))
        arrays["x"] = np.exp(0.5 * x) if exp else 2.0 * x
        t = {key: torch.tensor(v, dtype=torch.float64) for key, v in arrays.items()}
        t["_T"] = T

        def model():
            hmm = build(t, exp)
            if indep:
                hmm = dist.IndependentHMM(hmm)
            return pyro.sample("hmm", hmm, obs=t["x"])

        rep = LinearHMMReparam(**{p: StudentTReparam() for p in parts})
        torch.manual_seed(2000 + k)
        tr = poutine.trace(poutine.reparam(model, config={"hmm": rep})).get_trace()
        tr.compute_log_prob()
        sites = [s for s, site in tr.nodes.items() if site["type"] == "sample"]
        print("rep", name, {s: float(tr.nodes[s]["log_prob"].sum()) for s in sites})
        for key, v in arrays.items():
            flat["rep/%s/%s" % (name, key)] = v
        flat["rep/%s/sites" % name] = np.array(sites)
        for s in sites:
            if s != "hmm":
                flat["rep/%s/value_%s" % (name, s)] = tr.nodes[s]["value"].detach().numpy()
            flat["rep/%s/log_prob_%s" % (name, s)] = tr.nodes[s]["log_prob"].detach().numpy()


def main():
    rng = np.random.default_rng(20261019)
    flat = {}
    draw_cases(rng, flat)
    rep_cases(rng, flat)
    path = os.path.join(HERE, "linear_hmm.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
