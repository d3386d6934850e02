"""infer_discrete's chain route on the host (the oracle standing in for the device, the float64 restatement of
tests/chain_decode_cases.py standing in for kernels.logchain_decode): which models reach the kernel and with which
shapes, that its values are joint maximisers / exact posterior draws / the generic route's values, and how the uniforms
are reserved."""
import pytest
import torch

from tests import assign_cases as ac
from tests import chain_decode_cases as cc


@pytest.fixture
def chain_calls(oracle_backend, monkeypatch):
    """calls of kernels.logchain_decode as (B, T, K, mode, step_blocks)"""
    from pyro_amd import kernels
    from pyro_amd.infer import discrete

    calls = []
    monkeypatch.setattr(kernels, "logchain_decode", cc.decode_standin(calls), raising=False)
    monkeypatch.setattr(discrete, "_chain_decode_ready", lambda t: True, raising=False)
    return calls


def _infer(monkeypatch, fused, model, temperature, first_available_dim=-1, seed=2):
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import infer_discrete

    monkeypatch.setattr(c, "FUSED_CHAIN", fused)
    pyro.set_rng_seed(seed)
    return infer_discrete(model, first_available_dim=first_available_dim, temperature=temperature)()


def _stack(xs):
    return torch.stack([x.reshape(-1) for x in xs], -1)            # [B, T]


@pytest.mark.parametrize("temperature", [0, 1])
def test_a_markov_chain_makes_one_call_for_its_sites(chain_calls, monkeypatch, temperature):
    T = ac.hmm_tensors(5, 3, seed=0)
    fast = _infer(monkeypatch, True, ac.make_hmm(T), temperature)
    assert chain_calls == [(1, 5, 3, temperature, temperature)]    # (one float64 sequence: one block per step)
    assert all(x.shape == () and x.dtype == torch.int64 for x in fast)
    generic = _infer(monkeypatch, False, ac.make_hmm(T), temperature)
    assert len(chain_calls) == 1
    assert all(g.shape == () for g in generic) and torch.equal(_stack(fast), _stack(generic))


@pytest.mark.parametrize("temperature", [0, 1])
def test_a_vectorised_plate_of_chains_makes_one_call(chain_calls, monkeypatch, temperature):
    B = 3
    T = ac.hmm_tensors(5, 3, seed=1)
    T["data"] = torch.randint(0, 4, (B, 5), generator=torch.Generator().manual_seed(5))
    model = cc.make_plated_hmm(T, B)
    fast = _infer(monkeypatch, True, model, temperature, -2)
    assert chain_calls == [(B, 5, 3, temperature, 2 * temperature)]
    generic = _infer(monkeypatch, False, model, temperature, -2)
    assert len(chain_calls) == 1
    assert all(x.shape == (B,) for x in fast) and all(x.shape == (B,) for x in generic)
    assert torch.equal(_stack(fast), _stack(generic)) and len(torch.unique(_stack(fast))) > 1


def _tree_model(T):
    import pyro_amd as pyro
    import pyro_amd.distributions as dist

    def model():
        root = pyro.sample("x_0", dist.Categorical(T["init"]), infer={"enumerate": "parallel"})
        out = [root]
        for i in range(1, 4):
            x = pyro.sample("x_{}".format(i), dist.Categorical(T["tp"][root]), infer={"enumerate": "parallel"})
            pyro.sample("y_{}".format(i), dist.Categorical(T["ep"][x]), obs=T["data"][i])
            out.append(x)
        return out

    return model


@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("form", ["conditioned", "tree", "K65", "switch"])
def test_forms_that_stay_on_the_generic_route(chain_calls, monkeypatch, form, temperature):
    from pyro_amd import poutine

    T = ac.hmm_tensors(5, 65 if form == "K65" else 3, seed=2)
    model = ac.make_hmm(T)
    if form == "conditioned":
        model = poutine.condition(model, data={"x_2": torch.tensor(1)})
    elif form == "tree":
        model = _tree_model(T)
    xs = _infer(monkeypatch, form != "switch", model, temperature, -1)
    assert chain_calls == [] and len(xs) in (4, 5)


def test_map_is_a_joint_maximiser(chain_calls, monkeypatch):
    for seed in range(4):
        T = ac.hmm_tensors(5, 3, seed=seed)
        xs = _stack(_infer(monkeypatch, True, ac.make_hmm(T), 0))[0]
        best = ac.hmm_log_joint(T, ac.all_configs([3] * 5)).max()
        assert abs(float(ac.hmm_log_joint(T, xs) - best)) <= 1e-12 * abs(float(best))
    assert len(chain_calls) == 4


def test_map_under_exact_ties_is_still_a_joint_maximiser(chain_calls, monkeypatch):
    """two identical states everywhere in a chain (the construction of tests/test_infer_discrete_host.py): every step
    has ties, the path is consistent all the same"""
    T = ac.hmm_tensors(5, 3, seed=3)
    T["tp"][:, 2], T["ep"][2], T["init"][2] = T["tp"][:, 1], T["ep"][1], T["init"][1]
    T["tp"][2] = T["tp"][1]
    xs = _stack(_infer(monkeypatch, True, ac.make_hmm(T), 0))[0]
    best = ac.hmm_log_joint(T, ac.all_configs([3] * 5)).max()
    assert abs(float(ac.hmm_log_joint(T, xs) - best)) <= 1e-12 * abs(float(best))
    assert len(chain_calls) == 1


def test_draws_follow_the_exact_joint_posterior(chain_calls, monkeypatch):
    """3^5 = 243 joint states, 4000 independent copies of the chain under a plate in ONE call: every empirical joint
    frequency within 5 binomial standard errors (the bound of tests/test_infer_discrete_host.py)."""
    copies = 4000
    T = ac.hmm_tensors(5, 3, seed=0)
    data = T["data"]
    T["data"] = data.expand(copies, 5)
    xs = _stack(_infer(monkeypatch, True, cc.make_plated_hmm(T, copies), 1, -2, seed=7))
    assert chain_calls == [(copies, 5, 3, 1, copies // 2)] and xs.shape == (copies, 5)
    code = (xs * (3 ** torch.arange(4, -1, -1))).sum(-1)
    emp = torch.bincount(code, minlength=243).double() / copies
    T["data"] = data
    post = torch.softmax(ac.hmm_log_joint(T, ac.all_configs([3] * 5)), 0)
    bound = 5.0 * torch.sqrt(post * (1 - post) / copies)
    assert bool(((emp - post).abs() <= bound).all()), ((emp - post).abs() / bound).max()


@pytest.mark.parametrize("B,blocks", [(3, 2), (4, 2), (5, 3)])
def test_uniforms_are_reserved_as_one_reservation_per_site_would_be(chain_calls, monkeypatch, B, blocks):
    from pyro_amd import rng

    T = ac.hmm_tensors(5, 3, seed=1)
    T["data"] = torch.randint(0, 4, (B, 5), generator=torch.Generator().manual_seed(5))
    _infer(monkeypatch, True, cc.make_plated_hmm(T, B), 1, -2)
    assert chain_calls == [(B, 5, 3, 1, blocks)] and rng._STATE["offset"] == 5 * blocks
    used = rng._STATE["offset"]
    _infer(monkeypatch, True, cc.make_plated_hmm(T, B), 0, -2)
    assert rng._STATE["offset"] == 0                               # (re-seeded; the most probable path draws nothing)
    _infer(monkeypatch, False, cc.make_plated_hmm(T, B), 1, -2)
    assert rng._STATE["offset"] == used                            # the generic route: five reservations of B


def test_the_dispatcher_op_answers_on_meta_tensors():
    """pyro_amd::logchain_decode beside pyro_amd::logchain: a typed schema and a shape function (no device here)"""
    from pyro_amd.csrc.build import build_library, build_torch_ops
    from pyro_amd.ops import torch_library

    build_library()
    build_torch_ops()
    assert torch_library.available() and "pyro_amd::logchain_decode" in torch_library.registered_ops()
    assert str(torch.ops.pyro_amd.logchain_decode.default._schema) == (
        "pyro_amd::logchain_decode(Tensor unary, Tensor pairwise, int mode, int seed, int offset, Tensor? offset_dev, "
        "int step_blocks) -> (Tensor z, Tensor log_norm)")
    m = lambda *sh, **kw: torch.empty(sh, device="meta", **kw)  # noqa: E731
    z, norm = torch.ops.pyro_amd.logchain_decode(m(5, 7, 3), m(1, 6, 3, 3), 1, 0, 0, None, 2)
    assert z.shape == (5, 7) and z.dtype == torch.int64 and norm.shape == (5,) and norm.dtype == torch.float32
