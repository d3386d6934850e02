"""Covariance functions of Gaussian-process models (the classes and arguments of pyro/contrib/gp/kernels; the code
is this package's): the stationary families ``RBF``, ``RationalQuadratic``, ``Exponential``, ``Matern32``,
``Matern52`` over ``Isotropy``; ``Constant``, ``WhiteNoise``, ``Linear``; ``Sum`` and ``Product``.

A stationary family has two routes, chosen in ``Isotropy.forward``.

Kernel route: ``FUSED_GP_KERNEL`` on, device tensors of one dtype (f32 / f64), 2-D inputs (made contiguous after
``active_dims`` are taken), ``D <= 64``, a lengthscale of 1 or D elements, one-element variance and scale_mixture.  ONE
launch of pa_gp_kernel_fwd (csrc/gp_kernel.hip) forms r2 by DIRECT DIFFERENCES and writes K once; its backward
recomputes everything from the inputs (K is not saved: the models add noise to its diagonal in place) and reads the
incoming gradient once per side that wants a gradient.

Torch route: everything else (CPU tensors, ``D > 64``, other dtypes, a batched lengthscale, the switch off) evaluates
the reference's formula in torch operators: ``r2 = X2 - 2 X Z^T + Z2``, clamped at 0, ``r = sqrt(r2 + 1e-12)``.

The two routes differ ON PURPOSE in how r2 is formed: the expansion cancels (in float32 it is wrong by 8e-4 for
``Exponential`` at nearby points and useless for inputs shifted by 1e3), differences do not.  They describe the same
function and agree to the conditioning of the expansion.  ``diag=True`` never launches.

GP training is eager: the modules close over their data, so an SVI step over them is not captured into a graph
(``util.train``, or ``SVI(..., hip_graph=False)``), and ``torch.linalg.cholesky`` synchronises in any case.
"""
import math
import numbers

import torch
from torch.distributions import constraints

from ...nn.module import PyroParam
from ...ops.torch_library import dispatcher_op as _dispatcher_op
from .parameterized import Parameterized

FUSED_GP_KERNEL = True            # device f32 / f64, D <= kernels.GP_KERNEL_MAX_D: pa_gp_kernel_fwd / pa_gp_kernel_bwd


@_dispatcher_op("gp_kernel")
class _StationaryCovariance(torch.autograd.Function):
    """K = variance * f(r2) in ONE launch; the gradient recomputes r2 and f from the saved INPUTS (the output may be
    modified in place by the caller), one pass over the incoming gradient per side."""

    @staticmethod
    def forward(ctx, x, z, lengthscale, variance, alpha, family):
        from ... import kernels
        ctx.family = family
        ctx.save_for_backward(x, z, lengthscale, variance, alpha)
        return kernels.gp_kernel_fwd(x, z, lengthscale.reshape(-1), variance.reshape(-1),
                                     None if alpha is None else alpha.reshape(-1), family)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ... import kernels
        x, z, lengthscale, variance, alpha = ctx.saved_tensors
        want = list(ctx.needs_input_grad[:5])
        gx, gz, gl, gv, ga = kernels.gp_kernel_bwd(x, z, lengthscale.reshape(-1), variance.reshape(-1),
                                                   None if alpha is None else alpha.reshape(-1), g, ctx.family, want)
        return (gx, gz, None if gl is None else gl.reshape(lengthscale.shape),
                None if gv is None else gv.reshape(variance.shape),
                None if ga is None else ga.reshape(alpha.shape), None)


class Kernel(Parameterized):
    """A covariance function over ``input_dim`` features, the columns ``active_dims`` of its inputs."""

    def __init__(self, input_dim, active_dims=None):
        super().__init__()
        if active_dims is None:
            active_dims = list(range(input_dim))
        elif input_dim != len(active_dims):
            raise ValueError("Input size and the length of active dimensionals should be equal.")
        self.input_dim = input_dim
        self.active_dims = active_dims

    def forward(self, X, Z=None, diag=False):
        """The covariance matrix [N, M] of X [N, input_dim] and Z [M, input_dim] (Z = X when omitted), or with
        ``diag`` the diagonal [N] of K(X, X)."""
        raise NotImplementedError

    def _slice_input(self, X):
        if X.dim() == 2:
            return X[:, self.active_dims]
        if X.dim() == 1:
            return X.unsqueeze(1)
        raise ValueError("Input X must be either 1 or 2 dimensional.")


class _Combination(Kernel):
    def __init__(self, kern0, kern1):
        if not isinstance(kern0, Kernel):
            raise TypeError("The first component of a combined kernel must be a Kernel instance.")
        if not isinstance(kern1, (Kernel, numbers.Number)):
            raise TypeError("The second component of a combined kernel must be a Kernel instance or a number.")
        dims = set(kern0.active_dims)
        if isinstance(kern1, Kernel):
            dims |= set(kern1.active_dims)
        dims = sorted(dims)
        super().__init__(len(dims), dims)
        self.kern0 = kern0
        self.kern1 = kern1

    def _second(self, X, Z, diag):
        return self.kern1(X, Z, diag=diag) if isinstance(self.kern1, Kernel) else self.kern1


class Sum(_Combination):
    """``kern0 + kern1``; the second may be a number."""

    def forward(self, X, Z=None, diag=False):
        return self.kern0(X, Z, diag=diag) + self._second(X, Z, diag)


class Product(_Combination):
    """``kern0 * kern1``; the second may be a number."""

    def forward(self, X, Z=None, diag=False):
        return self.kern0(X, Z, diag=diag) * self._second(X, Z, diag)


Combination = _Combination


# ---- stationary families ---------------------------------------------------------------------------------------------
class Isotropy(Kernel):
    """Kernels that are functions of |x - z| / lengthscale.  A lengthscale of ``input_dim`` elements gives every
    feature its own (ARD)."""

    _family = None                # the kernel route's family (kernels.GP_FAMILIES), None: torch route only

    def __init__(self, input_dim, variance=None, lengthscale=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)
        lengthscale = torch.tensor(1.0) if lengthscale is None else lengthscale
        self.lengthscale = PyroParam(lengthscale, constraints.positive)

    # the torch route: the reference's expansion
    def _square_scaled_dist(self, X, Z=None):
        if Z is None:
            Z = X
        X, Z = self._slice_input(X), self._slice_input(Z)
        if X.size(1) != Z.size(1):
            raise ValueError("Inputs must have the same number of features.")
        sx, sz = X / self.lengthscale, Z / self.lengthscale
        x2, z2 = (sx ** 2).sum(1, keepdim=True), (sz ** 2).sum(1, keepdim=True)
        return (x2 - 2 * sx.matmul(sz.t()) + z2.t()).clamp(min=0)

    def _scaled_dist(self, X, Z=None):
        return (self._square_scaled_dist(X, Z) + 1e-12).sqrt()

    def _diag(self, X):
        return self.variance.expand(X.size(0))

    def _shape_parameter(self):
        return None

    def _fused(self, X, Z):
        """The contiguous sliced inputs and the parameters when the kernel route applies, else None."""
        if not FUSED_GP_KERNEL or self._family is None:
            return None
        variance, lengthscale, alpha = self.variance, self.lengthscale, self._shape_parameter()
        tensors = [X, variance, lengthscale] + ([] if Z is None else [Z]) + ([] if alpha is None else [alpha])
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == X.dtype for t in tensors):
            return None
        if X.dtype not in (torch.float32, torch.float64) or X.dim() > 2 or (Z is not None and Z.dim() > 2):
            return None
        Xs = self._slice_input(X).contiguous()
        Zs = None if Z is None else self._slice_input(Z).contiguous()
        D = Xs.size(1)
        if Zs is not None and Zs.size(1) != D:
            raise ValueError("Inputs must have the same number of features.")
        from ... import kernels as hip
        if not 1 <= D <= hip.GP_KERNEL_MAX_D or lengthscale.numel() not in (1, D) or lengthscale.dim() > 1:
            return None
        if variance.numel() != 1 or (alpha is not None and alpha.numel() != 1):
            return None
        return Xs, Zs, lengthscale, variance, alpha

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self._diag(X)
        fused = self._fused(X, Z)
        if fused is not None:
            return _StationaryCovariance.invoke(*fused, self._family)
        return self._torch_forward(X, Z)


class RBF(Isotropy):
    """variance * exp(-r2 / 2) (the squared exponential)."""
    _family = "rbf"

    def _torch_forward(self, X, Z):
        return self.variance * torch.exp(-0.5 * self._square_scaled_dist(X, Z))


class RationalQuadratic(Isotropy):
    """variance * (1 + r2 / (2 scale_mixture))^(-scale_mixture)."""
    _family = "rational_quadratic"

    def __init__(self, input_dim, variance=None, lengthscale=None, scale_mixture=None, active_dims=None):
        super().__init__(input_dim, variance, lengthscale, active_dims)
        scale_mixture = torch.tensor(1.0) if scale_mixture is None else scale_mixture
        self.scale_mixture = PyroParam(scale_mixture, constraints.positive)

    def _shape_parameter(self):
        return self.scale_mixture

    def _torch_forward(self, X, Z):
        r2 = self._square_scaled_dist(X, Z)
        return self.variance * (1 + (0.5 / self.scale_mixture) * r2).pow(-self.scale_mixture)


class Exponential(Isotropy):
    """variance * exp(-r)."""
    _family = "exponential"

    def _torch_forward(self, X, Z):
        return self.variance * torch.exp(-self._scaled_dist(X, Z))


class Matern32(Isotropy):
    """variance * (1 + sqrt(3) r) exp(-sqrt(3) r)."""
    _family = "matern32"

    def _torch_forward(self, X, Z):
        sr = math.sqrt(3.0) * self._scaled_dist(X, Z)
        return self.variance * (1 + sr) * torch.exp(-sr)


class Matern52(Isotropy):
    """variance * (1 + sqrt(5) r + 5/3 r2) exp(-sqrt(5) r)."""
    _family = "matern52"

    def _torch_forward(self, X, Z):
        r2 = self._square_scaled_dist(X, Z)
        sr = math.sqrt(5.0) * (r2 + 1e-12).sqrt()
        return self.variance * (1 + sr + (5.0 / 3.0) * r2) * torch.exp(-sr)


# ---- kernels that do not depend on a distance ----------------------------------------------------------------------
class Constant(Kernel):
    """k(x, z) = variance."""

    def __init__(self, input_dim, variance=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self.variance.expand(X.size(0))
        if Z is None:
            Z = X
        return self.variance.expand(X.size(0), Z.size(0))


class WhiteNoise(Kernel):
    """k(x, z) = variance where x and z are the same input point (Z omitted), else 0."""

    def __init__(self, input_dim, variance=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self.variance.expand(X.size(0))
        if Z is None:
            return self.variance.expand(X.size(0)).diag()
        return X.new_zeros(X.size(0), Z.size(0))


class Linear(Kernel):
    """k(x, z) = variance * x . z."""

    def __init__(self, input_dim, variance=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)

    def forward(self, X, Z=None, diag=False):
        X = self._slice_input(X)
        if diag:
            return self.variance * (X ** 2).sum(-1)
        Z = X if Z is None else self._slice_input(Z)
        if X.size(1) != Z.size(1):
            raise ValueError("Inputs must have the same number of features.")
        return self.variance * X.matmul(Z.t())
