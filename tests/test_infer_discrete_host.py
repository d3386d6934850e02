"""infer_discrete on the host (the oracle standing in for the device, float64 torch stand-ins for
kernels.mixture_assign*): joint maximisers and draws against brute-force enumeration, against the unmodified
reference (tests/golden/infer_discrete.npz), which mixtures reach the assignment kernels and with which arguments, the
API, and TraceEnum_ELBO.sample_posterior's fixed-seed draws from before the two shared their machinery
(tests/golden/sample_posterior_kat.npz)."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import assign_cases as ac
from tests.event_mixture_cases import FAMILIES, dist_id

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, K = 40, 3


@pytest.fixture
def assign_calls(oracle_backend, monkeypatch):
    """calls of the two kernels as (kernel, a's shape, a's strides, mode[, family id])"""
    from pyro_amd import kernels

    calls = []
    scalar, diag = ac.standins(calls)
    monkeypatch.setattr(kernels, "mixture_assign", scalar)
    monkeypatch.setattr(kernels, "mixture_assign_diag_normal", diag)
    return calls


def _infer(monkeypatch, fused, model, temperature, first_available_dim=-3, seed=2):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import infer_discrete

    monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
    pyro.set_rng_seed(seed)
    return infer_discrete(model, first_available_dim=first_available_dim, temperature=temperature)()


# ---- brute force -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_map_of_a_plated_mixture_is_a_joint_maximiser(assign_calls, monkeypatch, fused):
    T = ac.gmm_tensors(5, 3, seed=1)
    z = _infer(monkeypatch, fused, ac.make_gmm(T), 0, -2)
    assert z.shape == (5,) and len(assign_calls) == int(fused)
    best = ac.gmm_log_joint(T, ac.all_configs([3] * 5)).max()
    assert abs(float(ac.gmm_log_joint(T, z) - best)) <= 1e-12 * abs(float(best))


def test_map_of_a_markov_chain_is_a_viterbi_path(assign_calls, monkeypatch):
    T = ac.hmm_tensors(5, 3, seed=0)
    xs = _infer(monkeypatch, True, ac.make_hmm(T), 0, -1)
    xs = torch.stack([x.reshape(()) for x in xs])
    best = ac.hmm_log_joint(T, ac.all_configs([3] * 5)).max()
    assert abs(float(ac.hmm_log_joint(T, xs) - best)) <= 1e-12 * abs(float(best))
    assert not assign_calls


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_map_of_a_global_site_over_a_plated_local_site(assign_calls, monkeypatch, seed):
    T = ac.global_local_tensors(seed)
    s, z = _infer(monkeypatch, True, ac.make_global_local(T), 0, -2)
    cfg = ac.all_configs([2, 3, 3, 3])
    best = ac.global_local_log_joint(T, cfg[:, 0], cfg[:, 1:]).max()
    got = ac.global_local_log_joint(T, s.reshape(()), z.reshape(3))
    assert abs(float(got - best)) <= 1e-12 * abs(float(best))


def test_map_under_exact_ties_is_still_a_joint_maximiser(assign_calls, monkeypatch):
    """two identical states everywhere in a chain: every step has ties, the path is consistent all the same"""
    T = ac.hmm_tensors(5, 3, seed=3)
    T["tp"][:, 2], T["ep"][2], T["init"][2] = T["tp"][:, 1], T["ep"][1], T["init"][1]
    T["tp"][2] = T["tp"][1]
    xs = _infer(monkeypatch, True, ac.make_hmm(T), 0, -1)
    xs = torch.stack([x.reshape(()) for x in xs])
    best = ac.hmm_log_joint(T, ac.all_configs([3] * 5)).max()
    assert abs(float(ac.hmm_log_joint(T, xs) - best)) <= 1e-12 * abs(float(best))


def test_draws_follow_the_exact_joint_posterior(assign_calls, monkeypatch):
    """2 x 2 x 2 = 8 joint states (a global site over two rows of a local one), 20 000 independent copies under an
    outer plate in ONE call: every empirical joint frequency within 5 binomial standard errors, <= 0.018."""
    copies = 20_000
    T = ac.global_local_tensors(seed=4, rows=2, vals=2)
    s, z = _infer(monkeypatch, True, ac.make_global_local(T, copies=copies), 1, -3, seed=7)
    assert s.shape == (copies, 1) and z.shape == (copies, 2)
    code = s.reshape(-1).long() * 4 + z[:, 0] * 2 + z[:, 1]
    emp = torch.bincount(code, minlength=8).double() / copies
    cfg = ac.all_configs([2, 2, 2])
    post = torch.softmax(ac.global_local_log_joint(T, cfg[:, 0], cfg[:, 1:]), 0)
    bound = 5.0 * torch.sqrt(post * (1 - post) / copies)
    assert float(bound.max()) <= 0.018
    assert bool(((emp - post).abs() <= bound).all()), (emp, post)


# ---- against the unmodified reference ------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(GOLDEN_DIR, "infer_discrete.npz"))


def _same_as_reference(scores, got, want, lj_got, lj_want):
    """the same joint log-probability to 1e-9, the same indices wherever the reference's top two scores differ by
    more than 1e-6"""
    assert abs(lj_got - lj_want) <= 1e-9 * max(1.0, abs(lj_want)), (lj_got, lj_want)
    top = np.sort(scores, -1)
    decided = top[..., -1] - top[..., -2] > 1e-6
    assert np.array_equal(np.asarray(got)[decided], np.asarray(want)[decided])


@pytest.mark.parametrize("fused", [False, True])
def test_map_of_a_mixture_equals_the_references(assign_calls, monkeypatch, fused):
    g = _golden()
    T = {k: torch.as_tensor(g["gmm/" + k]) for k in ("data", "pi", "locs", "scale")}
    z = _infer(monkeypatch, fused, ac.make_gmm(T), 0, -2)
    want = torch.as_tensor(g["gmm/z"])
    scores = (torch.distributions.Normal(T["locs"], T["scale"]).log_prob(T["data"][:, None]) + T["pi"].log()).numpy()
    _same_as_reference(scores, z.numpy(), want.numpy(), float(ac.gmm_log_joint(T, z)),
                       float(ac.gmm_log_joint(T, want)))


def test_viterbi_path_equals_the_references(assign_calls, monkeypatch):
    g = _golden()
    T = {k: torch.as_tensor(g["hmm/" + k]) for k in ("init", "tp", "ep", "data")}
    xs = torch.stack([x.reshape(()) for x in _infer(monkeypatch, True, ac.make_hmm(T), 0, -1)])
    want = torch.as_tensor(g["hmm/xs"])
    lj = ac.hmm_log_joint(T, ac.all_configs([3] * 5))
    assert abs(float(ac.hmm_log_joint(T, xs) - ac.hmm_log_joint(T, want))) <= 1e-9
    top = torch.sort(lj).values
    if float(top[-1] - top[-2]) > 1e-6:             # (the path as a whole is what the reference maximises)
        assert torch.equal(xs, want)


# ---- routing ---------------------------------------------------------------------------------------------------------
def _both_routes(assign_calls, monkeypatch, model):
    """-> the calls of the fast route at temperature 0 and 1; asserts that the generic route makes none and returns
    the same values (at temperature 1 from the same uniforms)"""
    seen = []
    for temperature in (0, 1):
        del assign_calls[:]
        fast = _infer(monkeypatch, True, model, temperature)
        seen.append(list(assign_calls))
        generic = _infer(monkeypatch, False, model, temperature)
        assert len(assign_calls) == len(seen[-1])
        assert fast.dtype == generic.dtype == torch.int64 and torch.equal(fast, generic)
        assert not seen[-1] or len(torch.unique(fast)) > 1     # (the kernels' cases are no trivial ones)
    return seen


@pytest.mark.parametrize("family", FAMILIES)
def test_every_scalar_family_reaches_the_kernel(assign_calls, monkeypatch, family):
    seen = _both_routes(assign_calls, monkeypatch, ac.fitted_mixture("plain", "cpu", torch.float64, N, K,
                                                                     family=family))
    for temperature, calls in enumerate(seen):
        assert calls == [("scalar", (1, K), (K, 1), temperature, dist_id(family))] or \
            calls == [("scalar", (1, K), (1, 1), temperature, dist_id(family))], calls


@pytest.mark.parametrize("D", [2, 8])
@pytest.mark.parametrize("form", ["plain", "gate"])
def test_diagonal_normal_reaches_the_kernel(assign_calls, monkeypatch, form, D):
    seen = _both_routes(assign_calls, monkeypatch, ac.fitted_mixture(form, "cpu", torch.float64, N, K, D=D))
    for temperature, calls in enumerate(seen):
        assert len(calls) == 1 and calls[0][0] == "diag" and calls[0][3] == temperature, calls
        assert calls[0][1] == ((1, K) if form == "plain" else (1, N, K))


@pytest.mark.parametrize("form", ["gate", "grouped"])
def test_per_row_weights_reach_the_kernel_as_the_view_they_are(assign_calls, monkeypatch, form):
    seen = _both_routes(assign_calls, monkeypatch, ac.fitted_mixture(form, "cpu", torch.float64, N, K))
    for temperature, calls in enumerate(seen):
        assert len(calls) == 1 and calls[0][:2] == ("scalar", (1, N, K)) and calls[0][3] == temperature, calls
        assert calls[0][2][1:] == (K, 1), calls      # row-major [N, K] memory: no copy


@pytest.mark.parametrize("D", [None, 3])
def test_vectorised_parameter_sets_make_one_call(assign_calls, monkeypatch, D):
    B = 3
    model = ac.fitted_mixture("sets", "cpu", torch.float64, N, K, B, D=D)
    seen = _both_routes(assign_calls, monkeypatch, model)
    for temperature, calls in enumerate(seen):
        assert len(calls) == 1 and calls[0][0] == ("scalar" if D is None else "diag"), calls
        assert calls[0][1] == (B, K) and calls[0][2][0] == 0 and calls[0][3] == temperature, calls
    assert _infer(monkeypatch, True, model, 0).shape == (B, N)


@pytest.mark.parametrize("form,D,family,k", [("plain", 9, "Normal", K), ("mvn", 3, "Normal", K),
                                             ("plain", 3, "Bernoulli", K), ("plain", None, "Normal", 65),
                                             ("second", None, "Normal", K)])
def test_forms_that_stay_on_the_generic_route(assign_calls, monkeypatch, form, D, family, k):
    model = ac.fitted_mixture(form, "cpu", torch.float64, N, k, D=D, family=family)
    assert _both_routes(assign_calls, monkeypatch, model) == [[], []]


def test_fused_mixture_switch_turns_the_fast_route_off(assign_calls, monkeypatch):
    model = ac.fitted_mixture("plain", "cpu", torch.float64, N, K)
    _infer(monkeypatch, False, model, 0)
    _infer(monkeypatch, False, model, 1)
    assert not assign_calls


# ---- API -------------------------------------------------------------------------------------------------------------
def test_wrapper_and_both_decorator_forms(assign_calls):
    import pyro_amd as pyro
    from pyro_amd.infer import infer_discrete

    T = ac.gmm_tensors(7, 3, seed=2)
    model = ac.make_gmm(T)
    want = infer_discrete(model, first_available_dim=-2, temperature=0)()

    @infer_discrete(first_available_dim=-2, temperature=0)
    def decorated():
        return model()

    assert torch.equal(decorated(), want)
    from functools import partial

    @partial(infer_discrete, first_available_dim=-2, temperature=0)
    def wrapped():
        return model()

    assert torch.equal(wrapped(), want)
    assert pyro.infer.infer_discrete is infer_discrete


def test_arguments_are_checked(assign_calls):
    from pyro_amd.infer import infer_discrete

    model = ac.make_gmm(ac.gmm_tensors(7, 3, seed=2))
    with pytest.raises(ValueError, match="temperature"):
        infer_discrete(model, first_available_dim=-2, temperature=2)
    with pytest.raises(ValueError, match="first_available_dim"):
        infer_discrete(model, first_available_dim=1, temperature=0)
    with pytest.raises(ValueError, match="first_available_dim"):
        infer_discrete(model, temperature=0)


def test_no_enumerated_site_warns_under_strict_enumeration_warning(assign_calls):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd.infer import infer_discrete

    def model():
        return pyro.sample("z", dist.Categorical(torch.tensor([0.2, 0.8], dtype=torch.float64)))

    with pytest.warns(UserWarning, match="no sample sites configured for enumeration"):
        infer_discrete(model, first_available_dim=-1, temperature=0)()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        infer_discrete(model, first_available_dim=-1, temperature=0, strict_enumeration_warning=False)()


def test_continuous_sites_come_from_poutine_replay(assign_calls):
    """the assignment follows the replayed location: data at +-3, the replayed ``loc`` decides which component is
    which"""
    import pyro_amd as pyro
    import pyro_amd.distributions as dist
    from pyro_amd import poutine
    from pyro_amd.infer import infer_discrete

    data = torch.tensor([-3.1, -2.9, 3.0, 3.2, -3.0], dtype=torch.float64)

    def model():
        loc = pyro.sample("loc", dist.Normal(torch.zeros(2, dtype=torch.float64), 10.0).to_event(1))
        with pyro.plate("data", 5):
            z = pyro.sample("z", dist.Categorical(torch.tensor([0.5, 0.5], dtype=torch.float64)),
                            infer={"enumerate": "parallel"})
            pyro.sample("obs", dist.Normal(loc[z], 1.0), obs=data)
        return loc, z

    for locs, want in (([-3.0, 3.0], [0, 0, 1, 1, 0]), ([3.0, -3.0], [1, 1, 0, 0, 1])):
        def guide():
            pyro.sample("loc", dist.Delta(torch.tensor(locs, dtype=torch.float64)).to_event(1))

        guide_trace = poutine.trace(guide).get_trace()
        for temperature in (0, 1):
            loc, z = infer_discrete(poutine.replay(model, trace=guide_trace), first_available_dim=-2,
                                    temperature=temperature)()
            assert loc.tolist() == locs and z.tolist() == want


def test_sample_posterior_draws_are_what_they_were(oracle_backend):
    g = np.load(os.path.join(GOLDEN_DIR, "sample_posterior_kat.npz"))
    got = ac.sample_posterior_draws()
    assert set(got) == set(g.files)
    for k in g.files:
        assert np.array_equal(got[k], g[k]), k
