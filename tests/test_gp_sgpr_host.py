"""The streamed sparse-GP route without a device: its M x M algebra (models.streamed_log_prob / streamed_factors) on
statistics from plain torch against the dense route in float64, within 16 N 2^-52 cond(Kuu + jitter I) (1 + max|value|);
and the launch plan's invariants through the C-ABI's workspace query."""
import numpy as np
import pytest
import torch

from . import gp_cases as gc


def model_data(which):
    if which == "fixture":
        return gc.fixture_data()
    g = np.random.default_rng(5)
    X = g.standard_normal((300, 3))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    return {"X": t(X), "y": t(np.sin(X[:, 0]) + 0.1 * g.standard_normal(300)), "Xu": t(X[::9][:33] + 0.01),
            "Xnew": t(g.standard_normal((7, 3)))}


def dense_loss_and_grads(model):
    """-log p(y) of the dense route from torch.distributions (Trace_ELBO's loss for an empty guide), and its gradients."""
    import torch.distributions as td
    for p in model.parameters():
        p.grad = None
    model.set_mode("model")
    N = model.X.size(0)
    _, Wt = model._inducing()
    W = Wt.t()
    loss = -td.LowRankMultivariateNormal(model.X.new_zeros(N) + model.mean_function(model.X), W,
                                         model.noise.expand(N)).log_prob(model.y).sum()
    if model.approx == "VFE":
        loss = loss + ((model.kernel(model.X, diag=True) - W.pow(2).sum(-1)).sum() / model.noise).clamp(min=0) / 2
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}


@pytest.mark.parametrize("case", ["few_rows", "fixture", "two_outputs", "mean_function"])
@pytest.mark.parametrize("approx", ["VFE", "DTC"])
def test_streamed_algebra_against_the_dense_route(approx, case):
    from pyro_amd.contrib import gp
    models = gp.models
    data = model_data("fixture" if case == "fixture" else "few_rows")
    y = torch.stack((data["y"], data["y"].flip(0) * 0.5)) if case == "two_outputs" else None
    import pyro_amd as pyro
    dense = gc.build_model(gp, "sgpr_" + approx, data, y=y)
    pyro.clear_param_store()      # (a second model of the same names: the store would hand it the first one's Xu)
    model = gc.build_model(gp, "sgpr_" + approx, data, y=y)
    if case == "mean_function":
        dense.mean_function = model.mean_function = lambda X: 0.3 * X[:, 0] - 0.1
    want_loss, want_grads = dense_loss_and_grads(dense)

    def statistics(m):
        N = m.X.size(0)
        Kuu = m.kernel(m.Xu).contiguous()
        Luu = torch.linalg.cholesky(models._add_to_diagonal(Kuu, m.jitter))
        Kuf = m.kernel(m.Xu, m.X)
        r = (m.y - m.mean_function(m.X)).reshape(-1, N).t()
        return Luu, Kuf @ Kuf.t(), Kuf @ r, r

    for p in model.parameters():
        p.grad = None
    model.set_mode("model")
    Luu, A, b, r = statistics(model)
    N = model.X.size(0)
    log_prob, trace_term = models.streamed_log_prob(Luu, A, b, r.pow(2).sum(), model.kernel(model.X, diag=True).sum(),
                                                    model.noise, N, approx)
    assert (trace_term is None) == (approx == "DTC")
    loss = -(log_prob if trace_term is None else log_prob - trace_term / 2.0)
    loss.backward()
    with torch.no_grad():
        Kuu = model.kernel(model.Xu) + model.jitter * torch.eye(model.Xu.size(0), dtype=torch.float64)
        cond = torch.linalg.cond(Kuu).item()
    bound = lambda v: 16 * N * gc.EPS64 * cond * (1 + np.abs(v).max())      # noqa: E731
    assert abs(float(loss.detach()) - want_loss) <= bound(want_loss)
    for name, p in model.named_parameters():
        assert np.abs(p.grad.numpy() - want_grads[name]).max() <= bound(want_grads[name]), name
    with torch.no_grad():                                  # forward's two products: W D^-1 W^T = C / s, W D^-1 r = c / s
        model.set_mode("guide")
        Luu, A, b, r = statistics(model)
        C, c, LB = models.streamed_factors(Luu, A, b, model.noise)
        W = torch.linalg.solve_triangular(Luu, model.kernel(model.Xu, model.X), upper=False)
        for got, want in ((C / model.noise, (W / model.noise) @ W.t()), (c / model.noise, (W / model.noise) @ r),
                          (LB @ LB.t(), torch.eye(C.size(0), dtype=torch.float64) + (W / model.noise) @ W.t())):
            assert (got - want).abs().max().item() <= bound(want.numpy())


@pytest.mark.parametrize("N,M,D,Q,forced", [(1, 1, 1, 1, 0), (33, 129, 3, 2, 3), (4133, 257, 8, 16, 0),
                                            (10 ** 6, 32, 8, 1, 0), (10 ** 5, 512, 64, 16, 7)])
def test_workspace_follows_the_plan(N, M, D, Q, forced):
    from pyro_amd import _lib
    lib = _lib.load()
    f32, f64 = 0, 1
    query = lib.pa_gp_sgpr_workspace
    for dt, elem, tm, max_m in ((f32, 4, 128, 512), (f64, 8, 64, 256)):
        fwd = query(dt, N, M, D, Q, 0, 0, 0, forced)
        if M > max_m:
            assert fwd == 0
            continue
        blocks = -(-M // tm)
        pairs, rd = blocks * (blocks + 1) // 2, min(M, tm)
        per_split = 8 * (pairs * rd * rd + blocks * rd * Q)
        assert fwd > 0 and fwd % per_split == 0
        splits = fwd // per_split
        assert 1 <= splits <= -(-N // 32) and (not forced or splits == min(forced, -(-N // 32)))
        s_bytes = (M * M * elem + 7) // 8 * 8
        none = query(dt, N, M, D, Q, 1, 0, 0, forced)
        rows = query(dt, N, M, D, Q, 1, 0, 1, forced)
        both = query(dt, N, M, D, Q, 1, 1, 1, forced)
        chunks = -(-M // 128)
        assert both - rows == 8 * chunks * N * D
        assert (rows - none) % (8 * M * D) == 0 and (none - s_bytes) % (8 * chunks * (3 + D)) == 0
        assert (rows - none) // (8 * M * D) == (none - s_bytes) // (8 * chunks * (3 + D))      # the same splits
    assert query(f32, N, M, 65, Q, 0, 0, 0, 0) == 0 and query(f32, N, M, D, 17, 0, 0, 0, 0) == 0
