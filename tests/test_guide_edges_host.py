"""The numpy oracles of the step's last kernels (oracle/adam.py, oracle/gamma.py and the mvn / site functions of
tests/oracle_backend.py) against the references and under the tolerance rule of tests/guide_edge_cases.py, on
the CPU: pins the restatements the rest of the suite leans on, and checks that the float32 comparison formulas
of the rule leave at most 5 % of any case unscored."""
import numpy as np
import pytest
import torch

from oracle import adam as o_adam
from oracle import gamma as o_gamma
from tests import guide_edge_cases as gc
from tests import oracle_backend as ob

BOTH = [pytest.param(False, id="adam"), pytest.param(True, id="clipped")]


def _oracle_step(c):
    hy = c["hy"]
    with np.errstate(all="ignore"):
        return o_adam.adam_step(c["p"], c["g"], c["m"], c["v"], c["step0"] + 1, hy["lr"], hy["betas"], hy["eps"],
                                hy["wd"], hy["clip"], hy["lrd"], c["clipped"])


def _adam_variants(clipped):
    return [(0, 1, v) for v in ("zero", "zero_state", "naninf", "big", "lr0wd")]


# ---- Adam ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clipped", BOTH)
def test_adam_oracle_single_steps(clipped):
    """oracle.adam.adam_step against torch.optim.Adam / the recorded ClippedAdam on every hyper-parameter set
    and preset step count, and on the edge gradients: parameter and both moments per element."""
    keys = [(h, s, None) for h, s in gc.adam_single_keys(clipped)] + _adam_variants(clipped)
    for h, step0, variant in keys:
        c = gc.adam_case(clipped, h, step0, gc.ADAM_POOL, False, variant)
        gc.adam_check("host/clipped" if clipped else "host/adam", _oracle_step(c), c, False)


def test_recorded_hyper_parameters_are_the_case_module_s():
    z = gc.golden("adam_edges")
    hypers = gc.adam_hypers(True)
    for h, step0 in gc.adam_single_keys(True):
        hy = hypers[h]
        want = [hy["lr"], *hy["betas"], hy["eps"], hy["wd"], hy["clip"], hy["lrd"], step0]
        assert z[gc.adam_golden_key(h, step0) + "/hy"].tolist() == want
    for k, x in gc.make_adam_pool().items():
        assert np.array_equal(z["pool/" + k], x)
    hy = gc.ADAM_LR0WD_HYPER
    assert z["C/v_lr0wd/hy"].tolist() == [hy["lr"], *hy["betas"], hy["eps"], hy["wd"], hy["clip"], hy["lrd"], 1]


def test_the_float32_comparison_formula_of_clipped_adam_is_the_reference_s():
    """torch_clipped_adam_step (the cpu32 of the rule) in float64 against the recorded reference."""
    for h, step0 in gc.adam_single_keys(True):
        c = gc.adam_case(True, h, step0, gc.ADAM_POOL, False)
        got = gc.torch_clipped_adam_step(c["p"], c["g"], c["m"], c["v"], step0, c["hy"], gc.F64)
        gc.adam_check("host/clipped_torch", got, c, False)


@pytest.mark.parametrize("clipped", BOTH)
def test_adam_oracle_trajectory(clipped):
    p, grads, want = gc.adam_trajectory(clipped)
    hy = gc.ADAM_TRAJ_HYPER
    m, v = np.zeros_like(p), np.zeros_like(p)
    for s, g in enumerate(grads):
        M = gc.adam_magnitudes(p, g, m, v, s, hy, clipped, want[s][2])
        p, m, v = o_adam.adam_step(p, g, m, v, s + 1, hy["lr"], hy["betas"], hy["eps"], hy["wd"],
                                   hy["clip"] if clipped else 0.0, hy["lrd"] if clipped else 1.0, clipped)
        for what, got, ref, Mx in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), want[s], M):
            gc.check("host/traj", what, got, ref, Mx, False)


@pytest.mark.parametrize("clipped", BOTH)
def test_adam_float32_cases_stay_under_the_unscored_cap(clipped):
    keys = [(h, s, None) for h, s in gc.adam_single_keys(clipped)] + _adam_variants(clipped)
    for h, step0, variant in keys:
        c = gc.adam_case(clipped, h, step0, 257, True, variant)
        for r, c32 in zip(c["ref"], c["cpu32"]):
            assert gc.unscored_fraction(r, c32) <= gc.UNSCORED_CAP, (h, step0, variant)
    c = gc.adam_case(False, 0, 1, 257, True, "big")
    assert np.isinf(c["cpu32"][2]).sum() == 12 and np.isfinite(c["ref"][2]).all()


def test_oracle_backend_adam_step_moves_the_counter_and_zeroes_on_request():
    c = gc.adam_case(True, 5, gc.adam_step0_of(True, 5), gc.ADAM_POOL, False)
    hy = c["hy"]
    for zero in (True, False):
        p, g, m, v = (torch.tensor(c[k]) for k in "pgmv")
        step = torch.tensor([c["step0"], 0])
        ob.adam_step(p, g, m, v, step, hy["lr"], hy["betas"], hy["eps"], hy["wd"], hy["clip"], hy["lrd"], True,
                     zero_grad=zero)
        gc.adam_check("host/clipped", (p.numpy(), m.numpy(), v.numpy()), c, False)
        assert step.tolist() == [c["step0"] + 1, 0]
        assert (g == 0).all() if zero else np.array_equal(g.numpy(), c["g"])


# ---- Gamma ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_gamma_fixture_holds_the_grid(f32):
    a, x, ref = gc.gamma_grad_fixture(f32)
    ga, gx, quantile = gc.gamma_grid(f32, with_quantile_mask=True)
    assert np.array_equal(a, ga) and np.isfinite(ref).all() and (ref > 0).all()
    # x = a + 1, the sigma points, the a (1 +- r) points and the clamps are arithmetic on a: exact; the quantiles come
    # from scipy's inverse and may move in the last places between releases
    assert np.array_equal(x[~quantile], gx[~quantile])
    ulp = np.finfo(np.float32 if f32 else np.float64).eps
    assert (np.abs(x - gx)[quantile] <= 4 * ulp * x[quantile]).all()
    assert a.size > 200
    if f32:
        assert np.array_equal(gc.to32(a), a) and np.array_equal(gc.to32(x), x)
    for b in gc.GAMMA_BRANCHES:
        assert (gc.gamma_branch(a, x) == b).sum() >= 20


def test_gamma_oracle_gradient_per_branch():
    """oracle.gamma.implicit_grad against the 60-digit fixture: the measured relative error per branch is what
    GAMMA_HOST_MAX records (the device bound is 4 x that), and leaves the device bound under its cap of 1e-9."""
    worst = {b: 0.0 for b in gc.GAMMA_BRANCHES}
    for f32 in (False, True):
        a, x, ref = gc.gamma_grad_fixture(f32)
        got = o_gamma.implicit_grad(a, x)
        tiny = 2.0 ** -1022
        rel = np.where(got == ref, 0.0, np.abs(got - ref) / np.maximum(np.abs(ref), tiny))
        br = gc.gamma_branch(a, x)
        for b in gc.GAMMA_BRANCHES:
            keep = (br == b) & (np.abs(ref) > 1e-290)          # (a subnormal reference holds few digits)
            worst[b] = max(worst[b], float(rel[keep].max()))
            assert (np.abs(got - ref)[(br == b) & ~keep] <= 1e-290 * gc.GAMMA_HOST_MAX[b]).all()
    print("\nhost oracle, largest relative error per branch:", {b: "%.3g" % w for b, w in worst.items()})
    for b, w in worst.items():
        assert w <= gc.GAMMA_HOST_MAX[b], (b, w)
        assert w >= 0.25 * gc.GAMMA_HOST_MAX[b], "GAMMA_HOST_MAX[%s] is stale: measured %.3g" % (b, w)
        assert 4 * gc.GAMMA_HOST_MAX[b] <= gc.GAMMA_DEVICE_CAP


def test_gamma_grid_straddles_every_seam_and_the_oracle_does_not_jump_there():
    """Each seam of csrc/gamma.hip -- x = a + 1, |x - a| = 8 sqrt(a) from a = 1e4 on, a = 1e4, a = 1e8, and above
    a = 1e8 |x - a| = a / 100 on both sides of the mean -- has fixture points on both sides that take different
    evaluations, and across it the oracle's step differs from the fixture's by no more than the two evaluations'
    measured errors together."""
    a, x, ref = gc.gamma_grad_fixture(False)
    got = o_gamma.implicit_grad(a, x)
    br = gc.gamma_branch(a, x)

    def pair(i, j, want):
        assert {br[i], br[j]} == set(want), (a[i], x[i], a[j], x[j], br[i], br[j])
        jump = abs((got[i] - got[j]) - (ref[i] - ref[j]))
        assert jump <= (gc.GAMMA_HOST_MAX[br[i]] + gc.GAMMA_HOST_MAX[br[j]]) * max(abs(ref[i]), abs(ref[j]))

    def at(av, xv):
        i = np.flatnonzero((a == av) & (x == xv))
        assert i.size == 1, (av, xv)
        return int(i[0])

    hi = float(np.nextafter(1e8, np.inf))
    for av in (0.3, 30.0, 9999.0):                                     # x = a + 1
        pair(at(av, float(np.nextafter(av + 1.0, 0.0))), at(av, av + 1.0), ("series", "fraction"))
    for av in (1e4, 1e7, 1e8):                                          # 8 standard deviations
        s = np.sqrt(av)
        pair(at(av, av - 7.99 * s), at(av, av - 8.01 * s), ("cornish", "series"))
        pair(at(av, av + 7.99 * s), at(av, av + 8.01 * s), ("cornish", "fraction"))
    for lo_a, hi_a, sg, want in ((1e4 * (1 - 1e-12), 1e4, -7.99, ("series", "cornish")),       # a = 1e4
                                 (1e4 * (1 - 1e-12), 1e4, 7.99, ("fraction", "cornish")),
                                 (1e8, hi, -12.0, ("series", "cornish")),                   # a = 1e8
                                 (1e8, hi, 12.0, ("fraction", "cornish"))):
        pair(at(lo_a, lo_a + sg * np.sqrt(lo_a)), at(hi_a, hi_a + sg * np.sqrt(hi_a)), want)
    for av in (hi, 3e8):                                                # |x - a| = a / 100
        pair(at(av, av * (1 - 0.00999)), at(av, av * (1 - 0.01001)), ("cornish", "series"))
        pair(at(av, av * (1 + 0.00999)), at(av, av * (1 + 0.01001)), ("cornish", "fraction"))
        for r in (0.05, 0.09, 0.3):
            assert br[at(av, av * (1 - r))] == "series" and br[at(av, av * (1 + r))] == "fraction"
        assert br[at(av, av - 50 * np.sqrt(av))] == br[at(av, av * 1.005)] == "cornish"


def test_gamma_oracle_returns_nan_at_once_for_an_infinite_argument():
    import time
    t = time.time()
    got = o_gamma.implicit_grad([3.0, 3e8, np.inf, np.inf], [np.inf, np.inf, 5.0, np.inf])
    assert np.isnan(got).all() and time.time() - t < 1.0
    assert o_gamma.implicit_grad([np.nan, 3.0], [1.0, np.nan]).tolist() == [0.0, 0.0]     # (as before: not > 0)


def test_gamma_oracle_draws_pass_ks_at_the_device_test_s_seeds():
    from scipy import stats
    ps = {}
    for a in gc.GAMMA_KS_A:
        x = o_gamma.standard_gamma(np.full(gc.GAMMA_KS_N, a), gc.GAMMA_KS_SEED, gc.GAMMA_KS_OFFSET)
        ps[a] = stats.kstest(x, stats.gamma(a).cdf).pvalue
    print("\nKS p-values of the oracle's draws:", {a: "%.2f" % p for a, p in ps.items()})
    assert min(ps.values()) > gc.GAMMA_KS_P, ps


# ---- full-covariance guide -------------------------------------------------------------------------------

MVN_HOST = [(n, P) for n in gc.MVN_N for P in (1, 5, 13)]


@pytest.mark.parametrize("n,P", MVN_HOST)
def test_mvn_oracle_against_the_reference(n, P):
    """tests/oracle_backend.mvn_tril_sample / _bwd in float64.  z on every variant; log q and the backward where
    every rho is ordinary: the oracle solves the triangular system back from z - loc and divides by S, which the
    rule's M does not cover at rho = -30 or loc = 1e4 (see the case module)."""
    for variant in (None, "ordinary", "offset"):
        c = gc.mvn_case(n, P, False, variant)
        loc, rho, A, eps, d_z, d_q = c["inp"]
        z, logq, _ = ob.mvn_tril_sample(loc, rho, A, P, eps=eps)
        gc.mvn_check("host/mvn", (z.numpy(), None, None, None, None), c, False)
        if variant == "ordinary":
            d = ob.mvn_tril_sample_bwd(loc, rho, eps, z, d_z, d_q)
            gc.mvn_check("host/mvn", (None, logq.numpy()) + tuple(x.numpy() for x in d), c, False)
            assert (d[2].triu() == 0).all()


@pytest.mark.parametrize("n,P", [(2, 4), (65, 5), (129, 13)])
def test_mvn_direct_and_triangular_solve_forms_agree_where_rho_is_ordinary(n, P):
    """The backward's reference differentiates log q = -|eps|^2/2 - sum log S - n/2 log 2 pi; autograd through
    MultivariateNormal.log_prob(z) of the un-centred distribution is the same function: 1e-10 of the largest
    entry, the existing test's norm-wise tolerance."""
    loc, rho, A, eps, d_z, d_q = (x.clone() for x in gc.mvn_inputs(n, P, False, "ordinary"))
    direct = gc.mvn_case(n, P, False, "ordinary")["ref"]
    l, r, a = (x.requires_grad_(True) for x in (loc, rho, A))
    S = torch.nn.functional.softplus(r)
    T = S[:, None] * (a.tril(-1) + torch.eye(n, dtype=gc.F64))
    z = l + eps @ T.T
    lq = torch.distributions.MultivariateNormal(l, scale_tril=T).log_prob(z)
    ((z * d_z).sum() + (lq * d_q).sum()).backward()
    for got, ref in zip((z, lq, l.grad, r.grad, a.grad), direct):
        got = got.detach().numpy()
        assert np.abs(got - ref).max() <= 1e-10 * (np.abs(ref).max() + 1)


def test_mvn_float32_cases_stay_under_the_unscored_cap():
    for n in gc.MVN_N:
        for variant in (None, "offset"):
            c = gc.mvn_case(n, 13, True, variant)
            for r, c32 in zip(c["ref"], c["cpu32"]):
                assert gc.unscored_fraction(r, c32) <= gc.UNSCORED_CAP
    c = gc.mvn_case(65, 5, True, "underflow")
    assert gc.unscored_fraction(c["ref"][0], c["cpu32"][0]) == 0 and (c["cpu32"][1] == np.inf).all()


# ---- site kernels ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", gc.SITE_COLS)
def test_exp_site_oracle_and_the_float32_cap(cols):
    for rows in gc.SITE_ROWS + (gc.site_loop_rows(4),):
        for lower in gc.SITE_LOWER:
            c = gc.site_case(rows, cols, lower, False)
            value, ld = ob.exp_site_fwd(c["u"], cols, lower)
            gc.check("host/site", "value", value.numpy(), c["fwd"][0], c["M_fwd"][0], False)
            gc.check("host/site", "ld", ld.numpy(), c["fwd"][1], c["M_fwd"][1], False)
            assert ob.exp_site_fwd(c["u"], cols, lower, want_ld=False)[1] is None
            for which in ((True, True), (True, False), (False, True)):
                ref, _, M = gc.site_bwd_reference(c, which, False)
                got = ob.exp_site_bwd(c["value_in"], c["g_value"] if which[0] else None,
                                      c["g_ld"] if which[1] else None, cols, lower)
                gc.check("host/site", "g_u", got.numpy(), ref, M, False)
            c = gc.site_case(rows, cols, lower, True)
            for r, c32 in zip(c["fwd"], c["fwd32"]):
                assert gc.unscored_fraction(r, c32) <= gc.UNSCORED_CAP
            ref, c32, _ = gc.site_bwd_reference(c, (True, True), True)
            assert gc.unscored_fraction(ref, c32) <= gc.UNSCORED_CAP


@pytest.mark.parametrize("P,n", gc.SCORE_SHAPES)
def test_meanfield_score_oracle(P, n):
    c = gc.score_case(P, n, False)
    partial, gscale = ob.meanfield_score(c["z"], c["loc"], c["scale"], P, gc.SCORE_COEF)
    gc.score_check("host/score", partial.double().sum().numpy(), gscale.numpy(), c, False)
    c = gc.score_case(P, n, True)
    assert np.isfinite(c["cpu32"][0]) and np.isfinite(c["cpu32"][1]).all()
