"""gp.kernels.Polynomial and Coregionalize without a GPU: the torch routes against the reference fixture
(tests/golden/gp_dot.npz), the model over Sum(Polynomial, WhiteNoise), and the argument errors."""
import numpy as np
import pytest
import torch

import pyro_amd as pyro
import pyro_amd.contrib.gp as gp
from pyro_amd.infer import Trace_ELBO

from . import gp_cases as gc
from . import gp_dot_cases as dc
from .test_gp_host import _close, cpu_backend  # noqa: F401

GOLDEN = dict(np.load(dc.GOLDEN))
KERNELS = ["poly1", "poly2_active", "poly3", "coreg_low", "coreg_full"]


@pytest.mark.parametrize("kid", KERNELS)
def test_torch_route_matches_the_reference(kid):
    pyro.clear_param_store()      # (a plain Parameter, ``components``, is looked up by its name)
    data, kern = gc.fixture_data(), dc.kernel_table(gp)[kid]
    got = dc.record(kern, data["X"], data["Xnew"])
    assert sorted(got) == sorted(k.split("/")[2] for k in GOLDEN if k.startswith("kern/%s/" % kid))
    for name, value in got.items():
        _close(value, GOLDEN["kern/%s/%s" % (kid, name)])


def test_regression_loss_within_the_reference_sensitivity(cpu_backend):  # noqa: F811
    dc.check_model(gp, gc, Trace_ELBO())


@pytest.mark.parametrize("degree", [0, -2, 1.0, "2"])
def test_a_degree_that_is_no_positive_int(degree):
    with pytest.raises(ValueError, match="Degree for Polynomial kernel should be a positive integer."):
        gp.kernels.Polynomial(3, degree=degree)


def test_shape_errors_and_defaults():
    k = gp.kernels
    with pytest.raises(ValueError, match="Expected components.shape"):
        k.Coregionalize(3, components=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="Expected diagonal.shape"):
        k.Coregionalize(3, rank=2, diagonal=torch.ones(2))
    with pytest.raises(ValueError):
        k.Polynomial(3, active_dims=[0, 1])
    coreg = k.Coregionalize(4, rank=2)
    assert coreg.components.shape == (4, 2) and torch.equal(coreg.diagonal.detach(), torch.full((4,), 0.5))
    assert k.Coregionalize(3).components.shape == (3, 3)
    with pytest.raises(ValueError, match="same number of features"):
        k.Polynomial(2)(torch.zeros(4), torch.zeros(3, 2))      # one feature against two
    assert sorted(n for n, _ in k.Polynomial(2).named_parameters()) == ["bias_unconstrained", "variance_unconstrained"]
