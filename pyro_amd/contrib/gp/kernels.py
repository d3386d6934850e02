"""Covariance functions of Gaussian-process models (the classes and arguments of pyro/contrib/gp/kernels; the code
is this package's): the stationary families ``RBF``, ``RationalQuadratic``, ``Exponential``, ``Matern32``,
``Matern52`` over ``Isotropy``; ``Periodic``; ``Polynomial`` and ``Coregionalize``; ``Constant``, ``WhiteNoise``, ``Linear``; ``Sum`` and ``Product``;
``Cosine`` and ``Brownian``; ``Transforming`` with ``Exponent``, ``VerticalScaling`` and ``Warping``.

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

``Periodic`` has the same two routes under ``FUSED_GP_PERIODIC`` (csrc/gp_periodic.hip; a lengthscale and a period of 1
or D elements each).  Its torch route is the reference's formula with [N, M, D] temporaries, ``D`` times the size of
anything the kernel route allocates; both form the difference first, so they agree to the rounding of the angle.

``Polynomial`` and ``Coregionalize`` are functions of ``x . z``, which does not cancel, so their kernel route
(``FUSED_GP_DOT``, csrc/gp_dot.hip) forms the product on matrix cores: ONE launch writes ``variance * (bias + X Z^T)^degree``
once, the backward is one pass over the incoming gradient and nothing of size [N, M] is kept.  Conditions: those above,
one-element ``variance`` and ``bias``, ``degree <= 16``; ``Coregionalize`` runs it on the features ``[X C, X sqrt(d)]``
(``rank + input_dim <= 64``), which torch operators form so that autograd carries ``C`` and ``d``.  The torch route is the
reference's formula.  ``Linear`` stays one GEMM and a scale in torch; ``Polynomial(degree=1)`` is its fused, inhomogeneous
form.  ``Sum`` / ``Product`` and the sparse models see both classes as ordinary leaves.

``Sum`` and ``Product`` evaluate their children leaf by leaf and combine the [N, M] matrices with torch operators.  With
``FUSED_GP_COMPOSE`` on (opt-in: it saves 40-60 % of the peak memory and is faster at [4096, 4096], but was measured
up to 25 % slower at [512, 1e5]; README, "Gaussian processes") a tree is flattened into bias + sum_t coef_t prod_f leaf_f
-- products distributed over sums, numbers folded -- and every term whose leaves all meet the conditions of the kernel
routes above goes into ONE launch of pa_gp_compose_fwd (csrc/gp_compose.hip: at most 6 terms, 3 factors per term, 8
factors, a union of 64 columns), with one backward pass for all leaves; the other terms (``WhiteNoise``, ``Constant``,
``Linear``, what exceeds the caps) are evaluated as before and added.  Fewer than two such leaves, or ``diag=True``: as before.

``Cosine``, and ``Exponent``, ``Warping`` (its ``owarping_coef``) and ``VerticalScaling`` over a stationary leaf or
``Cosine``, stacked at most as ``VerticalScaling(q(leaf))``, are ONE launch of pa_gp_wrap_fwd (``FUSED_GP_WRAP``,
csrc/gp_wrap.hip): ``a_i q(variance f(r2_ij)) b_j`` with the leaf's own arithmetic, ``q`` the identity, ``exp`` or a
polynomial of at most 8 coefficients, ``a`` / ``b`` the values of ``vscaling_fn``, which torch operators form so that
autograd carries the gradient of the scale into the function, as it carries that of the points into ``iwarping_fn``.
The backward recomputes everything from the inputs; nothing of size [N, M] is kept.  The leaf must meet the conditions
of its kernel route.  Any other nesting, another child, ``diag=True``, more coefficients, or float64 with a polynomial
AND a scaling (that backward does not fit the registers) apply the reference's torch operators to what the child
returns.  ``Brownian`` has no kernel route.

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
FUSED_GP_PERIODIC = True          # the same conditions for Periodic: pa_gp_periodic_fwd / pa_gp_periodic_bwd
FUSED_GP_DOT = True               # the same conditions for Polynomial / Coregionalize: pa_gp_dot_fwd / pa_gp_dot_bwd
FUSED_GP_WRAP = True              # Cosine, and Exponent / Warping / VerticalScaling over a stationary leaf: pa_gp_wrap_*
FUSED_GP_COMPOSE = False          # opt-in: Sum / Product trees with two or more such leaves in ONE launch (pa_gp_compose_*)


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

    def forward(self, X, Z=None, diag=False):
        if not diag and FUSED_GP_COMPOSE:
            K = _composed(self, X, Z)
            if K is not None:
                return K
        return self._plain(X, Z, diag)


# ---- the composite route: a tree of Sum and Product as ONE sum of products -----------------------------------------
@_dispatcher_op("gp_compose")
class _ComposedCovariance(torch.autograd.Function):
    """K = bias + sum_t coef_t prod_f variance_f phi_f in ONE launch (csrc/gp_compose.hip); the gradient recomputes
    everything from the saved INPUTS (the output may be modified in place by the caller), one pass over the incoming
    gradient per side for all the leaves.  ``params``: variance, lengthscale and (where the leaf has one) scale_mixture
    or period of every factor, in the order of ``spec``."""

    @staticmethod
    def forward(ctx, spec, x, z, *params):
        from ... import kernels
        ctx.spec = spec
        ctx.save_for_backward(x, z, *params)
        return kernels.gp_compose_fwd(x, z, spec, _per_factor(spec, [p.reshape(-1) for p in params]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ... import kernels
        x, z, *params = ctx.saved_tensors
        needs = _per_factor(ctx.spec, list(ctx.needs_input_grad[3:]), False)
        gx, gz, grads = kernels.gp_compose_bwd(x, z, ctx.spec, _per_factor(ctx.spec, [p.reshape(-1) for p in params]), g,
                                               (ctx.needs_input_grad[1], ctx.needs_input_grad[2], needs))
        flat = [t for (kind, _), gs in zip(_factors_of(ctx.spec), grads) for t in gs[:_n_params(kind)]]
        return (None, gx, gz) + tuple(None if t is None else t.reshape(p.shape) for t, p in zip(flat, params))


def _factors_of(spec):
    return [f for _, fs in spec[1] for f in fs]


def _n_params(kind):
    return 3 if kind in ("rational_quadratic", "periodic") else 2


def _per_factor(spec, flat, fill=None):
    """The flat list (2 or 3 entries per factor) as one (variance, lengthscale, aux) per factor."""
    out, i = [], 0
    for kind, _ in _factors_of(spec):
        n = _n_params(kind)
        out.append(tuple(flat[i:i + n]) + (fill,) * (3 - n))
        i += n
    return out


def _normal_form(kern):
    """``kern`` as (terms, bias): terms a list of (coef, [leaf kernels]), products distributed over sums, numbers folded
    into coef and bias.  A product whose expansion would exceed the caps of the composite kernel stays one opaque
    leaf (it is then evaluated on its own, as before)."""
    if not isinstance(kern, _Combination):
        return [(1.0, [kern])], 0.0
    terms0, bias0 = _normal_form(kern.kern0)
    if isinstance(kern.kern1, Kernel):
        terms1, bias1 = _normal_form(kern.kern1)
    else:
        terms1, bias1 = [], float(kern.kern1)
    if isinstance(kern, Sum):
        return terms0 + terms1, bias0 + bias1
    from ... import kernels as hip
    terms = [(c0 * c1, f0 + f1) for c0, f0 in terms0 for c1, f1 in terms1]
    terms += [(c * bias1, f) for c, f in terms0 if bias1 != 0] + [(c * bias0, f) for c, f in terms1 if bias0 != 0]
    if len(terms) > hip.GP_COMPOSE_MAX_TERMS or any(len(f) > hip.GP_COMPOSE_MAX_TERM_FACTORS for _, f in terms):
        return [(1.0, [kern])], 0.0
    return terms, bias0 * bias1


def _leaf_parameters(leaf, X, Z):
    """(kind, parameters) of a leaf that the composite kernel takes -- the conditions of the leaf's own kernel route,
    without its copies of the inputs -- else None."""
    from ... import kernels as hip
    if isinstance(leaf, Isotropy) and leaf._family is not None and FUSED_GP_KERNEL:
        kind, aux = leaf._family, leaf._shape_parameter()
        sizes = (1,)
    elif isinstance(leaf, Periodic) and FUSED_GP_PERIODIC:
        kind, aux = "periodic", leaf.period
        sizes = (1, len(leaf.active_dims))
    else:
        return None
    variance, lengthscale, D = leaf.variance, leaf.lengthscale, len(leaf.active_dims)
    tensors = [variance, lengthscale] + ([] if aux is None else [aux])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == X.dtype and t.dim() <= 1 for t in tensors):
        return None
    if (not 1 <= D <= hip.GP_KERNEL_MAX_D or variance.numel() != 1 or lengthscale.numel() not in (1, D)
            or (aux is not None and aux.numel() not in sizes)):
        return None
    return kind, tensors


def _composed(kern, X, Z):
    """K(X, Z) of the tree under ``kern`` with every term of stationary and periodic leaves in ONE composite launch and
    the other terms (WhiteNoise, Constant, Linear, what is over the caps) evaluated as before and added; None when
    fewer than two leaves could share the launch, so that the tree is evaluated as before."""
    tensors = [X] + ([] if Z is None else [Z])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == X.dtype and t.dim() == 2 for t in tensors):
        return None
    if X.dtype not in (torch.float32, torch.float64) or (Z is not None and Z.size(1) != X.size(1)):
        return None
    from ... import kernels as hip
    terms, bias = _normal_form(kern)
    fused, rest, cache, columns, n_factors, sum_d = [], [], {}, set(), 0, 0
    for coef, leaves in terms:
        for leaf in leaves:
            if id(leaf) not in cache:
                cache[id(leaf)] = _leaf_parameters(leaf, X, Z)
        dims = set(d for leaf in leaves for d in leaf.active_dims)
        size = sum(len(leaf.active_dims) for leaf in leaves)
        if (all(cache[id(leaf)] is not None for leaf in leaves) and len(fused) < hip.GP_COMPOSE_MAX_TERMS
                and n_factors + len(leaves) <= hip.GP_COMPOSE_MAX_FACTORS and len(columns | dims) <= hip.GP_KERNEL_MAX_D
                and sum_d + size <= hip.GP_COMPOSE_MAX_SUM_D and max(dims) < X.size(1)):
            fused.append((coef, leaves))
            columns |= dims
            n_factors, sum_d = n_factors + len(leaves), sum_d + size
        else:
            rest.append((coef, leaves))
    if n_factors < 2:
        return None
    union = sorted(columns)
    where = {d: i for i, d in enumerate(union)}
    spec = (bias, tuple((coef, tuple((cache[id(leaf)][0], tuple(where[d] for d in leaf.active_dims)) for leaf in leaves))
                        for coef, leaves in fused))
    params = [p for _, leaves in fused for leaf in leaves for p in cache[id(leaf)][1]]
    whole = union == list(range(X.size(1)))
    Xs = (X if whole else X[:, union]).contiguous()
    Zs = None if Z is None else (Z if whole else Z[:, union]).contiguous()
    K = _ComposedCovariance.invoke(spec, Xs, Zs, *params)
    for coef, leaves in rest:
        term = leaves[0](X, Z)
        for leaf in leaves[1:]:
            term = term * leaf(X, Z)
        K = K + (term if coef == 1.0 else coef * term)
    return K


class Sum(_Combination):
    """``kern0 + kern1``; the second may be a number."""

    def _plain(self, X, Z, diag):
        return self.kern0(X, Z, diag=diag) + self._second(X, Z, diag)


class Product(_Combination):
    """``kern0 * kern1``; the second may be a number."""

    def _plain(self, X, Z, diag):
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
        return self._fused_inputs(X, Z)

    def _fused_inputs(self, X, Z):
        """The same without the switch and the family: the conditions on the tensors alone."""
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


# ---- the periodic kernel ---------------------------------------------------------------------------------------------
@_dispatcher_op("gp_periodic")
class _PeriodicCovariance(torch.autograd.Function):
    """K = variance * exp(-2 sum_k sin^2(pi (x - z) / p_k) / l_k^2) in ONE launch; the gradient recomputes K from the
    saved INPUTS (the output may be modified in place by the caller), one pass over the incoming gradient per side."""

    @staticmethod
    def forward(ctx, x, z, lengthscale, period, variance):
        from ... import kernels
        ctx.save_for_backward(x, z, lengthscale, period, variance)
        return kernels.gp_periodic_fwd(x, z, lengthscale.reshape(-1), period.reshape(-1), variance.reshape(-1))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ... import kernels
        x, z, lengthscale, period, variance = ctx.saved_tensors
        grads = kernels.gp_periodic_bwd(x, z, lengthscale.reshape(-1), period.reshape(-1), variance.reshape(-1), g,
                                        list(ctx.needs_input_grad[:5]))
        shapes = (None, None, lengthscale.shape, period.shape, variance.shape)
        return tuple(t if t is None or s is None else t.reshape(s) for t, s in zip(grads, shapes))


class Periodic(Kernel):
    """variance * exp(-2 sum_k sin^2(pi (x_k - z_k) / period_k) / lengthscale_k^2).  ``lengthscale`` and ``period`` have
    1 or ``input_dim`` elements, independently."""

    def __init__(self, input_dim, variance=None, lengthscale=None, period=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)
        lengthscale = torch.tensor(1.0) if lengthscale is None else lengthscale
        self.lengthscale = PyroParam(lengthscale, constraints.positive)
        period = torch.tensor(1.0) if period is None else period
        self.period = PyroParam(period, constraints.positive)

    def _fused(self, X, Z):
        """The contiguous sliced inputs and the parameters when the kernel route applies, else None."""
        if not FUSED_GP_PERIODIC:
            return None
        variance, lengthscale, period = self.variance, self.lengthscale, self.period
        tensors = [X, variance, lengthscale, period] + ([] if Z is None else [Z])
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
        if not 1 <= D <= hip.GP_KERNEL_MAX_D or variance.numel() != 1:
            return None
        if any(p.numel() not in (1, D) or p.dim() > 1 for p in (lengthscale, period)):
            return None
        return Xs, Zs, lengthscale, period, variance

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self.variance.expand(X.size(0))
        fused = self._fused(X, Z)
        if fused is not None:
            return _PeriodicCovariance.invoke(*fused)
        # the torch route: the reference's formula, with its [N, M, D] temporaries
        X = self._slice_input(X)
        Z = X if Z is None else self._slice_input(Z)
        if X.size(1) != Z.size(1):
            raise ValueError("Inputs must have the same number of features.")
        theta = (X[:, None, :] - Z[None, :, :]) * (math.pi / self.period)
        return self.variance * torch.exp(-2 * (torch.sin(theta) / self.lengthscale).pow(2).sum(-1))


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


# ---- kernels that are functions of x . z: the product on matrix cores -------------------------------------------------
@_dispatcher_op("gp_dot")
class _DotCovariance(torch.autograd.Function):
    """K = variance * (bias + x z^T)^degree in ONE launch (csrc/gp_dot.hip; bias None: 0, variance None: 1); the gradient
    recomputes K from the saved INPUTS (the output may be modified in place by the caller) in one pass over the incoming
    gradient."""

    @staticmethod
    def forward(ctx, x, z, variance, bias, degree):
        from ... import kernels
        ctx.degree = degree
        ctx.save_for_backward(x, z, variance, bias)
        flat = lambda t: None if t is None else t.reshape(-1)      # noqa: E731
        return kernels.gp_dot_fwd(x, z, flat(variance), flat(bias), degree)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ... import kernels
        x, z, variance, bias = ctx.saved_tensors
        flat = lambda t: None if t is None else t.reshape(-1)      # noqa: E731
        gx, gz, gv, gb = kernels.gp_dot_bwd(x, z, flat(variance), flat(bias), ctx.degree, g,
                                            list(ctx.needs_input_grad[:4]))
        return (gx, gz, None if gv is None else gv.reshape(variance.shape),
                None if gb is None else gb.reshape(bias.shape), None)


def _dot_inputs(kern, X, Z, parameters):
    """The contiguous sliced inputs when the dot kernel's route applies to them and to ``parameters`` (one-element
    tensors), else None."""
    if not FUSED_GP_DOT:
        return None
    tensors = [X] + list(parameters) + ([] if Z is None else [Z])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == X.dtype for t in tensors):
        return None
    if X.dtype not in (torch.float32, torch.float64) or X.dim() > 2 or (Z is not None and Z.dim() > 2):
        return None
    if any(p.numel() != 1 for p in parameters):
        return None
    Xs = kern._slice_input(X)
    Zs = None if Z is None else kern._slice_input(Z)
    if Zs is not None and Zs.size(1) != Xs.size(1):
        raise ValueError("Inputs must have the same number of features.")
    return Xs, Zs


class Polynomial(Kernel):
    """k(x, z) = variance * (bias + x . z)^degree, ``degree`` a positive int (degree 1: the inhomogeneous linear kernel)."""

    def __init__(self, input_dim, variance=None, bias=None, degree=1, active_dims=None):
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)
        bias = torch.tensor(1.0) if bias is None else bias
        self.bias = PyroParam(bias, constraints.positive)
        if not isinstance(degree, int) or degree < 1:
            raise ValueError("Degree for Polynomial kernel should be a positive integer.")
        self.degree = degree

    def _fused(self, X, Z):
        """The contiguous sliced inputs and the parameters when the kernel route applies, else None."""
        from ... import kernels as hip
        variance, bias = self.variance, self.bias
        sliced = _dot_inputs(self, X, Z, (variance, bias))
        if sliced is None or not 1 <= sliced[0].size(1) <= hip.GP_KERNEL_MAX_D or self.degree > hip.GP_DOT_MAX_DEGREE:
            return None
        Xs, Zs = sliced
        return Xs.contiguous(), None if Zs is None else Zs.contiguous(), variance, bias, self.degree

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self.variance * (self.bias + (self._slice_input(X) ** 2).sum(-1)) ** self.degree
        fused = self._fused(X, Z)
        if fused is not None:
            return _DotCovariance.invoke(*fused)
        # the torch route: the reference's formula, four passes over [N, M]
        X = self._slice_input(X)
        Z = X if Z is None else self._slice_input(Z)
        if X.size(1) != Z.size(1):
            raise ValueError("Inputs must have the same number of features.")
        return self.variance * (self.bias + X.matmul(Z.t())) ** self.degree


class Coregionalize(Kernel):
    """k(x, z) = x^T (C C^T + diag(d)) z, the linear model of coregionalization: ``components`` C [input_dim, rank] (drawn
    with E[C C^T] = I / 2 when only ``rank``, default ``input_dim``, is given) and a positive ``diagonal`` d [input_dim]
    (default 0.5)."""

    def __init__(self, input_dim, rank=None, components=None, diagonal=None, active_dims=None):
        super().__init__(input_dim, active_dims)
        if components is None:
            rank = input_dim if rank is None else rank
            components = torch.randn(input_dim, rank) * (0.5 / rank) ** 0.5
        else:
            rank = components.size(-1)
        if components.shape != (input_dim, rank):
            raise ValueError("Expected components.shape == ({},rank), actual {}".format(input_dim, components.shape))
        self.components = torch.nn.Parameter(components)
        diagonal = components.new_ones(input_dim) * 0.5 if diagonal is None else diagonal
        if diagonal.shape != (input_dim,):
            raise ValueError("Expected diagonal.shape == ({},), actual {}".format(input_dim, diagonal.shape))
        self.diagonal = PyroParam(diagonal, constraints.positive)

    def _fused(self, X, Z):
        """The features [X C, X sqrt(d)] of the kernel route ([N, rank + input_dim], formed by torch operators: autograd
        carries C and d) when it applies, else None."""
        from ... import kernels as hip
        components, diagonal = self.components, self.diagonal
        if not all(t.is_cuda and t.dtype == X.dtype for t in (components, diagonal)):
            return None
        if components.size(1) + components.size(0) > hip.GP_KERNEL_MAX_D:
            return None
        sliced = _dot_inputs(self, X, Z, ())
        if sliced is None:
            return None
        root = diagonal.sqrt()
        Xs, Zs = sliced
        return (torch.cat([Xs.matmul(components), Xs * root], 1),
                None if Zs is None else torch.cat([Zs.matmul(components), Zs * root], 1), None, None, 1)

    def forward(self, X, Z=None, diag=False):
        if not diag:
            fused = self._fused(X, Z)
            if fused is not None:
                return _DotCovariance.invoke(*fused)
        # the torch route: the reference's formula
        X = self._slice_input(X)
        Xc = X.matmul(self.components)
        if diag:
            return (Xc ** 2).sum(-1) + (X ** 2).mv(self.diagonal)
        if Z is None:
            Z, Zc = X, Xc
        else:
            Z = self._slice_input(Z)
            Zc = Z.matmul(self.components)
        return Xc.matmul(Zc.t()) + (X * self.diagonal).matmul(Z.t())


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


# ---- Cosine, Brownian ------------------------------------------------------------------------------------------------
@_dispatcher_op("gp_wrap")
class _WrappedCovariance(torch.autograd.Function):
    """K = a_i q(variance * f(r2_ij)) b_j in ONE launch (csrc/gp_wrap.hip); the gradient recomputes everything from the
    saved INPUTS (the output may be modified in place by the caller), one pass over the incoming gradient per side.
    ``q``: None, "exp" or a tuple of polynomial coefficients (constants: no gradient)."""

    @staticmethod
    def forward(ctx, x, z, lengthscale, variance, alpha, a, b, family, q):
        from ... import kernels
        ctx.family, ctx.q = family, q
        ctx.save_for_backward(x, z, lengthscale, variance, alpha, a, b)
        return kernels.gp_wrap_fwd(x, z, lengthscale.reshape(-1), variance.reshape(-1),
                                   None if alpha is None else alpha.reshape(-1), family, q, a, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ... import kernels
        x, z, lengthscale, variance, alpha, a, b = ctx.saved_tensors
        gx, gz, gl, gv, gal, ga, gb = kernels.gp_wrap_bwd(
            x, z, lengthscale.reshape(-1), variance.reshape(-1), None if alpha is None else alpha.reshape(-1), g,
            ctx.family, ctx.q, a, b, list(ctx.needs_input_grad[:7]))
        return (gx, gz, None if gl is None else gl.reshape(lengthscale.shape),
                None if gv is None else gv.reshape(variance.shape),
                None if gal is None else gal.reshape(alpha.shape), ga, gb, None, None)


class Cosine(Isotropy):
    """variance * cos(r).  Its kernel route is the wrapped covariance kernel's (``FUSED_GP_WRAP``) under the conditions
    of the stationary families; ``_family`` stays None, so that the composite and the streamed sparse routes treat it
    as a torch-route leaf."""

    def forward(self, X, Z=None, diag=False):
        if diag:
            return self._diag(X)
        fused = self._fused_inputs(X, Z) if FUSED_GP_WRAP else None
        if fused is not None:
            return _WrappedCovariance.invoke(*fused, None, None, "cosine", None)
        return self._torch_forward(X, Z)

    def _torch_forward(self, X, Z):
        return self.variance * torch.cos(self._scaled_dist(X, Z))


class Brownian(Kernel):
    """Two-sided Brownian motion over ONE feature: variance * min(|x|, |z|) where x and z have the same sign, else 0.
    No kernel route: it is one element-wise pass over [N, M] with nothing to fuse."""

    def __init__(self, input_dim, variance=None, active_dims=None):
        if input_dim != 1:
            raise ValueError("Input dimensional for Brownian kernel must be 1.")
        super().__init__(input_dim, active_dims)
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)

    def forward(self, X, Z=None, diag=False):
        X = self._slice_input(X)
        if diag:
            return self.variance * X.abs().squeeze(1)
        Zt = (X if Z is None else self._slice_input(Z)).t()
        if X.size(1) != Zt.size(0):
            raise ValueError("Inputs must have the same number of features.")
        return torch.where(X.sign() == Zt.sign(), self.variance * torch.min(X.abs(), Zt.abs()),
                           X.new_zeros(X.size(0), Zt.size(1)))


# ---- kernels derived from a kernel ---------------------------------------------------------------------------------------
def _horner(K, coef):
    value = coef[-1]
    for c in reversed(coef[:-1]):
        value = c + value * K
    return value


def _peel(kern):
    """``kern`` as (vscaling_fn, iwarping_fn, q, leaf) when it is VerticalScaling(q(leaf)) with either layer optional,
    q one of Exponent / Warping and the leaf a stationary kernel or Cosine -- what ONE wrapped launch evaluates -- else
    None.  A bare stationary leaf is None as well: it has a route of its own."""
    from ... import kernels as hip
    scale = warp = q = None
    if isinstance(kern, VerticalScaling):
        scale, kern = kern.vscaling_fn, kern.kern
    if isinstance(kern, Exponent):
        q, kern = "exp", kern.kern
    elif isinstance(kern, Warping):
        warp, q, kern = kern.iwarping_fn, kern.owarping_coef and tuple(kern.owarping_coef), kern.kern
    if not isinstance(kern, Isotropy):
        return None
    family = "cosine" if isinstance(kern, Cosine) else kern._family
    if family is None:
        return None
    if isinstance(q, tuple) and len(q) > hip.GP_WRAP_MAX_COEF:
        return None
    if q is None and scale is None and kern._family is not None:
        return None
    return scale, warp, q, kern, family


def _wrapped(kern, X, Z):
    """K(X, Z) of a tree that ``_peel`` takes, else None.  ``vscaling_fn`` and ``iwarping_fn`` are evaluated ONCE, with
    torch operators; where the leaf then meets the conditions of its kernel route the rest is one launch, otherwise the
    reference's operators are applied to the same pieces."""
    parts = _peel(kern)
    if parts is None:
        return None
    scale, warp, q, leaf, family = parts
    a = b = None
    if scale is not None:
        a, b = scale(X), None if Z is None else scale(Z)
    if warp is not None:
        X, Z = warp(X), None if Z is None else warp(Z)
    fused = leaf._fused_inputs(X, Z) if isinstance(leaf, Cosine) else leaf._fused(X, Z)
    if fused is not None:
        sizes = (fused[0].size(0), None if fused[1] is None else fused[1].size(0))
        scales_fit = all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == fused[0].dtype
                                       and tuple(t.shape) == (n,)) for t, n in zip((a, b), sizes))
        if scales_fit and not (isinstance(q, tuple) and a is not None and fused[0].dtype == torch.float64):
            return _WrappedCovariance.invoke(*fused, a, b, family, q)
    K = leaf(X, Z)
    K = K if q is None else (K.exp() if q == "exp" else _horner(K, q))
    return K if a is None else a.unsqueeze(1) * K * (a if b is None else b).unsqueeze(0)


class Transforming(Kernel):
    """Kernels derived from a kernel ``kern``; ``input_dim`` and ``active_dims`` are the child's."""

    def __init__(self, kern):
        if not isinstance(kern, Kernel):
            raise TypeError("The original kernel of a transforming kernel must be a Kernel instance.")
        super().__init__(kern.input_dim, kern.active_dims)
        self.kern = kern

    def forward(self, X, Z=None, diag=False):
        if not diag and FUSED_GP_WRAP:
            K = _wrapped(self, X, Z)
            if K is not None:
                return K
        return self._plain(X, Z, diag)

    def _child(self, X, Z, diag):
        """What the child returns.  A nesting that ONE launch does not take stays in torch operators down to its leaf:
        a child that is itself derived does not launch for its part of it."""
        if isinstance(self.kern, Transforming):
            return self.kern._plain(X, Z, diag)
        return self.kern(X, Z, diag=diag)


class Exponent(Transforming):
    """exp(k(x, z))."""

    def _plain(self, X, Z, diag):
        return self._child(X, Z, diag).exp()


class VerticalScaling(Transforming):
    """f(x) k(x, z) f(z) for a function ``vscaling_fn`` of the inputs that returns one number per point."""

    def __init__(self, kern, vscaling_fn):
        super().__init__(kern)
        self.vscaling_fn = vscaling_fn

    def _plain(self, X, Z, diag):
        a = self.vscaling_fn(X)
        if diag:
            return a * self._child(X, Z, diag) * a
        b = a if Z is None else self.vscaling_fn(Z)
        return a.unsqueeze(1) * self._child(X, Z, diag) * b.unsqueeze(0)


class Warping(Transforming):
    """q(k(f(x), f(z))): ``iwarping_fn`` f warps the inputs (deep kernel learning), ``owarping_coef`` are the
    coefficients of the polynomial q, lowest first: a list of non-negative ints, constants without a gradient.  (A
    negative coefficient is refused whatever its type; the reference lets a negative int pass.)"""

    def __init__(self, kern, iwarping_fn=None, owarping_coef=None):
        super().__init__(kern)
        self.iwarping_fn = iwarping_fn
        if owarping_coef is not None:
            if any(coef < 0 for coef in owarping_coef):
                raise ValueError("Coefficients of the polynomial must be a non-negative integer.")
            if len(owarping_coef) < 2 and sum(owarping_coef) == 0:
                raise ValueError("The ouput warping polynomial should have a degree of at least 1.")
        self.owarping_coef = owarping_coef

    def _plain(self, X, Z, diag):
        if self.iwarping_fn is not None:
            X, Z = self.iwarping_fn(X), None if Z is None else self.iwarping_fn(Z)
        K = self._child(X, Z, diag)
        return K if self.owarping_coef is None else _horner(K, self.owarping_coef)
