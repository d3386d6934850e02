"""gp.kernels.Cosine, Brownian, Exponent, VerticalScaling and Warping without a GPU: the torch routes against the
reference fixture (tests/golden/gp_wrap.npz), the argument errors, and that CPU tensors never reach the launchers."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.contrib.gp as gp

from . import gp_cases as gc
from . import gp_wrap_cases as wc
from .test_gp_host import _close

GOLDEN = dict(np.load(wc.GOLDEN))


def _weights():
    return {n: torch.as_tensor(GOLDEN["weights/" + n]).requires_grad_() for n in ("W", "c", "v")}


@pytest.mark.parametrize("kid", wc.KERNELS)
def test_torch_route_matches_the_reference(kid, monkeypatch):
    from pyro_amd import kernels

    def never(*a, **k):
        raise AssertionError("a CPU tensor reached the wrapped covariance launchers")
    monkeypatch.setattr(kernels, "gp_wrap_fwd", never)
    monkeypatch.setattr(kernels, "gp_wrap_bwd", never)
    pyro.clear_param_store()
    data, w = gc.fixture_data(), _weights()
    got = wc.record(wc.kernel_table(gp, w)[kid], data["X"], data["Xnew"], w)
    assert sorted(got) == sorted(k.split("/")[2] for k in GOLDEN if k.startswith("kern/%s/" % kid))
    for name, value in got.items():
        _close(value, GOLDEN["kern/%s/%s" % (kid, name)])


def test_argument_errors():
    k = gp.kernels
    with pytest.raises(ValueError, match="Input dimensional for Brownian kernel must be 1."):
        k.Brownian(2)
    with pytest.raises(ValueError, match="non-negative"):
        k.Warping(k.RBF(3), owarping_coef=[1, -1])
    with pytest.raises(ValueError, match="degree of at least 1"):
        k.Warping(k.RBF(3), owarping_coef=[0])
    for make in (k.Exponent, lambda c: k.VerticalScaling(c, torch.sin), k.Warping):
        with pytest.raises(TypeError):
            make(3.0)
    warped = k.Warping(k.RBF(2, active_dims=[0, 2]), owarping_coef=[0, 1])
    assert warped.input_dim == 2 and warped.active_dims == [0, 2] and k.Cosine._family is None
