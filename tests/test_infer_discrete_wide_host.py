"""infer_discrete's fast route for the wide leaves on the host (the oracle standing in for the device, float64 torch
stand-ins for kernels.mixture_assign_event / mixture_assign_mvn from tests/assign_wide_cases.py): which mixtures reach
which kernel, with which shapes and mode, which stay on the generic route, and that both routes return the same
values at both temperatures."""
import pytest
import torch

from tests import assign_cases as ac
from tests import assign_wide_cases as wc
from tests.event_mixture_cases import FAMILIES, TWO_PARAMETERS, dist_id

N, K, B = 40, 3, 3


@pytest.fixture
def wide_calls(oracle_backend, monkeypatch):
    """calls of the two kernels (see wide_standins), the wide route switched on for CPU tensors"""
    from pyro_amd import kernels
    from pyro_amd.infer import discrete

    calls = []
    event, mvn = wc.wide_standins(calls)
    monkeypatch.setattr(kernels, "mixture_assign_event", event)
    monkeypatch.setattr(kernels, "mixture_assign_mvn", mvn)
    monkeypatch.setattr(discrete, "_wide_assign_ready", lambda x: True)
    return calls


def _infer(monkeypatch, fused, model, temperature, seed=2):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import infer_discrete

    monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
    pyro.set_rng_seed(seed)
    return infer_discrete(model, first_available_dim=-3, temperature=temperature)()


def _both_routes(calls, monkeypatch, model):
    """-> the calls of the fast route at temperature 0 and 1; asserts that the generic route makes none and returns
    the same values (at temperature 1 from the same uniforms)"""
    seen = []
    for temperature in (0, 1):
        del calls[:]
        fast = _infer(monkeypatch, True, model, temperature)
        seen.append(list(calls))
        generic = _infer(monkeypatch, False, model, temperature)
        assert len(calls) == len(seen[-1])
        assert fast.dtype == generic.dtype == torch.int64 and torch.equal(fast, generic)
        assert not seen[-1] or len(torch.unique(fast)) > 1
    return seen


@pytest.mark.parametrize("form", ["plain", "sets"])
@pytest.mark.parametrize("family,D", [(f, 12) for f in FAMILIES] + [("Normal", 9), ("Bernoulli", 3),
                                      ("Bernoulli", 300)])
def test_event_shaped_mixtures_reach_the_event_kernel(wide_calls, monkeypatch, family, D, form):
    model = ac.fitted_mixture(form, "cpu", torch.float64, N, K, B, D=D, family=family)
    Bs = B if form == "sets" else 1
    p1 = (Bs, K, D) if family in TWO_PARAMETERS else None
    seen = _both_routes(wide_calls, monkeypatch, model)
    for temperature, calls in enumerate(seen):
        assert calls == [("event", dist_id(family), (N, D), (Bs, K), (Bs, K, D), p1, temperature)], calls
    assert _infer(monkeypatch, True, model, 0).shape == ((B, N) if form == "sets" else (N,))


@pytest.mark.parametrize("form", ["plain", "sets"])
@pytest.mark.parametrize("D", [3, 17])
def test_full_covariance_mixtures_reach_the_mvn_kernel(wide_calls, monkeypatch, form, D):
    model = wc.fitted_mvn_mixture(form, "cpu", torch.float64, N, K, B, D)
    Bs = B if form == "sets" else 1
    seen = _both_routes(wide_calls, monkeypatch, model)
    for temperature, calls in enumerate(seen):
        assert calls == [("mvn", (N, D), (Bs, K), (Bs, K, D), (Bs, K, D, D), temperature)], calls


def test_a_diagonal_scale_tril_reaches_the_mvn_kernel(wide_calls, monkeypatch):
    seen = _both_routes(wide_calls, monkeypatch, ac.fitted_mixture("mvn", "cpu", torch.float64, N, K, D=3))
    for temperature, calls in enumerate(seen):
        assert calls == [("mvn", (N, 3), (1, K), (1, K, 3), (1, K, 3, 3), temperature)], calls


def test_the_narrow_kernels_keep_their_mixtures(wide_calls, monkeypatch):
    """scalar data and a diagonal Normal over at most 8 features do not come here"""
    from pyro_amd import kernels

    narrow = []
    scalar, diag = ac.standins(narrow)
    monkeypatch.setattr(kernels, "mixture_assign", scalar)
    monkeypatch.setattr(kernels, "mixture_assign_diag_normal", diag)
    for D in (None, 8):
        _both_routes(wide_calls, monkeypatch, ac.fitted_mixture("plain", "cpu", torch.float64, N, K, D=D))
        assert not wide_calls
    assert [c[0] for c in narrow] == ["scalar", "scalar", "diag", "diag"]


@pytest.mark.parametrize("case", ["gate_bernoulli", "gate_normal", "gate_mvn", "event_1025", "mvn_65", "k_65"])
def test_forms_that_stay_on_the_generic_route(wide_calls, monkeypatch, case):
    """per-row weights, D over the kernels' limits and K = 65 make no call"""
    dt = torch.float64
    model = {"gate_bernoulli": lambda: ac.fitted_mixture("gate", "cpu", dt, N, K, D=12, family="Bernoulli"),
             "gate_normal": lambda: ac.fitted_mixture("gate", "cpu", dt, N, K, D=9),
             "gate_mvn": lambda: wc.fitted_mvn_mixture("gate", "cpu", dt, N, K, B, 3),
             "event_1025": lambda: ac.fitted_mixture("plain", "cpu", dt, 12, K, D=1025, family="Bernoulli"),
             "mvn_65": lambda: wc.fitted_mvn_mixture("plain", "cpu", dt, 12, K, B, 65),
             "k_65": lambda: ac.fitted_mixture("plain", "cpu", dt, 12, 65, D=9)}[case]()
    assert _both_routes(wide_calls, monkeypatch, model) == [[], []]


def test_cpu_tensors_make_no_call_by_default(oracle_backend, monkeypatch):
    """with the predicate as shipped (is the observation on the device?), CPU tensors stay on the generic route"""
    from pyro_amd import kernels
    from pyro_amd.infer import discrete

    assert discrete._wide_assign_ready(torch.zeros(2)) is False
    calls = []
    event, mvn = wc.wide_standins(calls)
    monkeypatch.setattr(kernels, "mixture_assign_event", event)
    monkeypatch.setattr(kernels, "mixture_assign_mvn", mvn)
    for model in (ac.fitted_mixture("plain", "cpu", torch.float64, N, K, D=9),
                  ac.fitted_mixture("plain", "cpu", torch.float64, N, K, D=3, family="Bernoulli"),
                  wc.fitted_mvn_mixture("plain", "cpu", torch.float64, N, K, B, 3)):
        assert _both_routes(calls, monkeypatch, model) == [[], []]
