"""Gaussian processes (reference: pyro/contrib/gp): ``Parameterized``, the kernel classes, exact and sparse GP
regression, ``VariationalSparseGP`` with the likelihoods, ``util.conditional`` and ``util.train``.  On the device the
stationary kernels form their covariance matrix and its gradient with csrc/gp_kernel.hip
(``kernels.FUSED_GP_KERNEL``) and ``Periodic`` with csrc/gp_periodic.hip (``kernels.FUSED_GP_PERIODIC``); a ``Sum`` /
``Product`` tree of them can take ONE launch of csrc/gp_compose.hip (``kernels.FUSED_GP_COMPOSE``, opt-in);
``Polynomial`` and ``Coregionalize`` form ``x . z`` on matrix cores with csrc/gp_dot.hip (``kernels.FUSED_GP_DOT``);
sparse regression and the sparse variational model stream their statistics over the data (csrc/gp_sgpr.hip,
csrc/gp_cond.hip).  ``Cosine``, and ``Exponent``, ``Warping`` and ``VerticalScaling`` over a stationary kernel, write
their matrix in ONE launch of csrc/gp_wrap.hip (``kernels.FUSED_GP_WRAP``); ``Brownian`` is torch operators only.

Not here: VariationalGP and GPLVM."""
from . import kernels, likelihoods, models, util
from .parameterized import Parameterized

__all__ = ["Parameterized", "kernels", "likelihoods", "models", "util"]
