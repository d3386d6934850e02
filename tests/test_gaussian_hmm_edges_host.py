"""The edge cases of tests/gaussian_hmm_edge_cases.py on the CPU: the float64 torch route of distributions/hmm.py
against the fixtures of the unmodified reference (tests/golden/gaussian_hmm_edges.npz) on every layout case, and the
conditions the device tests of tests/test_gaussian_hmm_edges_gpu.py rest on, checked on the torch route alone."""
import numpy as np
import pytest
import torch

from pyro_amd.distributions import hmm
from tests import gaussian_hmm_cases as gc
from tests import gaussian_hmm_edge_cases as ec
from tests import gaussian_hmm_prior_cases as pr

TOL64 = 1e-9
NARROW = [k for k in ec.A_KEYS if k[2:] == ec.A_WIDTHS[0]]


def test_the_layout_matrix_is_what_it_says():
    assert len(ec.LAYOUTS) == 26 and len(ec.A_KEYS) == 52
    seen = set()
    for key in ec.A_KEYS:
        per_series, per_step, init_shared = ec.LAYOUTS[key[1]]
        t = ec.inputs(key)
        h, o = key[2:]
        assert t["x"].shape == (ec.A_B, ec.A_T, o) and t["m0"].shape == (1 if init_shared else ec.A_B, h)
        for name, bs, st in zip(ec.TIMED, per_series, per_step):
            assert t[name].shape[:2] == (ec.A_B if bs else 1, ec.A_T if st else 1), (key, name)
        seen.add((per_series, per_step, init_shared))
    assert len(seen) == 26
    # no existing fixture layout among them: there all six agree on both axes
    assert all(len(set(ps)) == 2 or len(set(st)) == 2 for ps, st, _ in seen)


@pytest.mark.parametrize("key", NARROW, ids=lambda k: k[1])
def test_torch_route_float64_against_the_reference(key):
    g = ec.golden(key)
    for k in ec.NAMES:                                   # the generators reproduce the fixture's inputs
        assert np.array_equal(ec.inputs(key)[k], g[k]), k
    got = ec.cpu_route(key, ec.F64)
    assert ec.lp_err(got["log_prob"], g["log_prob"]) < TOL64
    for k in ec.NAMES:
        assert gc.rel_err(got["g_" + k], g["g_" + k]) < TOL64, k
    assert gc.rel_err(got["filter_mean"], g["filter_mean"]) < TOL64
    assert gc.rel_err(got["filter_cov"], g["filter_cov"]) < TOL64
    # _backward_sample_maps / _backward_sample: the last state's map is the filter's posterior, and a draw with zero
    # noise is the chain of the c's and G's
    c, G, L = got["c"], got["G"], got["L"]
    assert gc.rel_err(c[:, -1], g["filter_mean"]) < TOL64
    assert gc.rel_err(L[:, -1] @ np.swapaxes(L[:, -1], -1, -2), g["filter_cov"]) < TOL64
    assert not G[:, -1].any() and np.array_equal(L, np.tril(L))
    eps = ec.noise(key)[0].numpy()
    z = c[None, :, -1] + np.einsum("bij,sbj->sbi", L[:, -1], eps[:, :, -1])
    want = [z]
    for t in range(ec.A_T - 2, -1, -1):
        z = c[None, :, t] + np.einsum("bij,sbj->sbi", G[:, t], z) + np.einsum("bij,sbj->sbi", L[:, t], eps[:, :, t])
        want.append(z)
    assert gc.rel_err(got["draws"], np.stack(want[::-1], axis=2)) < 1e-12
    # the torch rsample against the numpy restatement of the three equations, every parameter expanded
    t = ec.leaves(key, ec.F64, ec.CPU)
    names = ("m0", "P0", "F", "q", "Q", "H", "r", "R")
    m = {}
    for k, p in zip(names, ec.parts(t)):
        lead = (ec.A_B,) if k in ("m0", "P0") else (ec.A_B, ec.A_T)
        m[k] = np.broadcast_to(p.numpy(), lead + tuple(p.shape[len(lead):]))
    wx, wz = pr.restate(m, *(e.numpy() for e in ec.noise(key)[1]))
    assert gc.rel_err(got["prior_x"], wx) < 1e-12 and gc.rel_err(got["prior_z"], wz) < 1e-12


@pytest.mark.parametrize("key", [k for k in ec.A_KEYS if k[2:] == ec.A_WIDTHS[1]][::5], ids=lambda k: k[1])
def test_wide_layout_cases_are_well_posed(key):
    got = ec.cpu_route(key, ec.F64)
    assert all(np.isfinite(v).all() for v in got.values())
    base = ec.errors(ec.cpu_route(key, ec.F32), got)
    assert set(base) == set(ec.KINDS) and max(base.values()) < 1e-4, base


@pytest.mark.parametrize("shape", ec.D_SHAPES, ids=lambda s: "h%d_o%d" % s)
@pytest.mark.parametrize("recipe", ec.RECIPES)
def test_ill_conditioned_float32_torch_route_is_finite(recipe, shape):
    """the condition of group D: the float32 torch route is finite on all eight seeds, so the base of the bound is"""
    worst = {}
    for key in ec.d_keys(recipe, shape):
        want, got = ec.cpu_route(key, ec.F64), ec.cpu_route(key, ec.F32)
        assert all(np.isfinite(v).all() for v in want.values()), key
        assert all(np.isfinite(v).all() for v in got.values()), key
        for kind, e in ec.errors(got, want).items():
            worst[kind] = max(worst.get(kind, 0.0), e)
    print(recipe, shape, "float32 torch route, worst of the seeds:", ec.fmt(worst))
    assert all(np.isfinite(e) for e in worst.values())


@pytest.mark.parametrize("key", ec.E_KEYS, ids=lambda k: "%s_h%d" % k[1:3])
def test_bad_pivot_cases_have_a_finite_log_prob(key):
    """the conditions of group E on the float64 torch route: the forward pass does not see the bad matrix"""
    p, x = ec.bad_pivot_parts(key, "Q", ec.F64, ec.CPU)
    assert np.linalg.eigvalsh(p[4][1].numpy()).min() < 0                          # Q of series 1 is not positive definite
    assert torch.isfinite(hmm._kalman_filter(*p, x)[0]).all()
    p, x = ec.bad_pivot_parts(key, "P0", ec.F64, ec.CPU)
    F0, Q = p[2][1, 0], p[4][1, 0]
    assert np.linalg.eigvalsh((F0.T @ p[1][1] @ F0 + Q).numpy()).min() > 0        # the first P^p
    assert torch.isfinite(hmm._kalman_filter(*p, x)[0]).all()
    for h, o in (key[2:],):
        t = ec.long_draw_inputs(h, o)
        assert t["Lq"].shape[:2] == (3, ec.E_LONG_T) and ec.E_LONG_BAD_STEP > 64


@pytest.mark.parametrize("kind", ["base", "one", "partly"])
@pytest.mark.parametrize("shape", ec.C_SHAPES, ids=lambda s: "h%d_o%d" % s)
def test_class_batch_plumbing_against_flat_parts(shape, kind):
    """group C's model on the CPU: the class over its broadcasting leaves gives what _kalman_filter gives on the same
    parameters expanded by hand to [B, T, ...] (the issue's combination agrees with the reference at 8.5e-14)"""
    h, o = shape
    t = ec.class_leaves(h, o, kind, ec.F64, ec.CPU)
    d, x = ec.class_build(t)
    batch = () if kind == "one" else (2, 3)
    if kind == "partly":                      # leads that are partly 1 reach _kernel_parts
        assert d._parts[2].shape[:-3] == (2, 1) and d._parts[5].shape[:-3] == (1, 3)
    assert d.batch_shape == batch and d.event_shape == (ec.C_T, o) and not x.is_contiguous()
    lp = d.log_prob(x)
    grads = torch.autograd.grad(lp.sum(), [t[k] for k in ec.C_NAMES])
    for k, g in zip(ec.C_NAMES, grads):
        assert g.shape == t[k].shape and torch.isfinite(g).all(), k
    cov = lambda L: L @ L.transpose(-1, -2)                                              # noqa: E731
    with torch.no_grad():
        T = ec.C_T
        F = t["Ft"].transpose(-1, -2).expand(batch + (T, h, h))
        flat = (t["m0"].expand(batch + (h,)), cov(t["L0"]).expand(batch + (h, h)), F, t["q"].expand(batch + (T, h)),
                cov(t["Lq"]).expand(batch + (T, h, h)), t["H"].expand(batch + (T, h, o)), t["r"].expand(batch + (T, o)),
                cov(t["Lr"]).expand(batch + (T, o, o)))
        want, m, P = hmm._kalman_filter(*(p.contiguous() for p in flat), x.contiguous())
        assert lp.shape == batch and gc.rel_err(lp.numpy(), want.numpy()) < 1e-12
        post = d.filter(x)
        assert gc.rel_err(post.loc.numpy(), m.numpy()) < 1e-12
        # one more leading dim on the value, and an expanded distribution
        x4 = torch.stack([x, x + 1.0, x - 1.0, 2.0 * x])
        assert d.log_prob(x4).shape == (4,) + batch and gc.rel_err(d.log_prob(x4)[0].numpy(), want.numpy()) < 1e-12
        e = d.expand((5,) + batch)
        assert e.batch_shape == (5,) + batch and gc.rel_err(e.log_prob(x)[4].numpy(), want.numpy()) < 1e-12
