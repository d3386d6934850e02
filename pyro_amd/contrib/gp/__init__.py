"""Gaussian processes (reference: pyro/contrib/gp): ``Parameterized``, the kernel classes, exact and sparse GP
regression, ``util.conditional`` and ``util.train``.  On the device the stationary kernels form their covariance matrix
and its gradient with csrc/gp_kernel.hip (``kernels.FUSED_GP_KERNEL``).

Not here: VariationalGP, VariationalSparseGP, GPLVM and the likelihoods; the Periodic, Cosine, Brownian, Polynomial,
Coregionalize, Exponent, VerticalScaling and Warping kernels."""
from . import kernels, models, util
from .parameterized import Parameterized

__all__ = ["Parameterized", "kernels", "models", "util"]
