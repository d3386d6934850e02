"""Gaussian-process models (the classes and arguments of pyro/contrib/gp/models; the code is this package's):
``GPModel``, exact ``GPRegression``, ``SparseGPRegression`` with the DTC, FITC and VFE approximations, and
``VariationalSparseGP`` with a likelihood of ``likelihoods``.

A model closes over its data: ``model()`` and ``guide()`` take no arguments, so an SVI step over them is eager (see
``util.train``).  Covariance matrices come from ``self.kernel``; on the device the stationary families form them in one
launch (``kernels.FUSED_GP_KERNEL``).  Noise and jitter are added to the diagonal of the matrix IN PLACE, as the
reference does; the fused kernel's backward recomputes what it needs from the inputs, so that is allowed.

``SparseGPRegression`` with DTC or VFE has a STREAMED route (``FUSED_SGPR``): the data enter the loss only through
A = Kuf Kuf^T [M, M], b = Kuf r [M, Q], sum r^2 and sum_n k(x_n, x_n), and csrc/gp_sgpr.hip forms A and b (and their
gradient) in one pass over X each way without Kuf [M, N] in memory; the rest is M x M algebra in torch
(``streamed_log_prob``).

``VariationalSparseGP`` needs the data only through the per-point marginals of f(X) given q(u), and has a STREAMED route
for them too (``FUSED_VSGP``): csrc/gp_cond.hip forms loc[q, n] = k_n . a_q and s[n, j] = |P_j k_n|^2 (k_n = Kuf[:, n])
one tile of 32 points at a time, with a [M, Q] and P [1 + Q, M, M] from M x M triangular solves in torch
(``conditional_factors``); nothing of size M x N exists in either direction.  ``forward(Xnew)`` takes the same route.
Float64 models only: float32 models run ``util.conditional`` (README "Gaussian processes" has the figures).
"""
import math

import torch
from torch.distributions import constraints
from torch.nn import Parameter

from ... import distributions as dist
from ... import poutine, primitives
from ...nn.module import PyroParam, pyro_method
from .kernels import Isotropy
from .parameterized import Parameterized
from . import util
from .util import conditional

FUSED_SGPR = True                 # SparseGPRegression, DTC / VFE: the statistics from pa_gp_sgpr_fwd / pa_gp_sgpr_bwd
FUSED_SGPR_MIN_N = 1000000        # ... from this many data points on (README "Gaussian processes": the sweep)
FUSED_VSGP = True                 # VariationalSparseGP: the marginals from pa_gp_cond_fwd / pa_gp_cond_bwd
FUSED_VSGP_MIN_N = float("inf")   # ... from this many points on (README "Gaussian processes": no swept N qualifies)


def _zero_mean_function(x):
    return 0


def _add_to_diagonal(matrix, value):
    """matrix [n, n] (contiguous) += value * I, in place; returns it."""
    n = matrix.size(-1)
    matrix.view(-1)[::n + 1] += value
    return matrix


class _StreamedStatistics(torch.autograd.Function):
    """(A, b) = (Kuf Kuf^T, Kuf r) with Kuf[i, n] = k(xu_i, x_n), in one pass over x; the gradient is one more pass
    (G = (gA + gA^T) Kuf + gb r^T exists only block by block inside the kernel).  No double backward."""

    @staticmethod
    def forward(ctx, x, xu, r, lengthscale, variance, alpha, family):
        from ... import kernels
        ctx.family = family
        ctx.save_for_backward(x, xu, r, lengthscale, variance, alpha)
        return kernels.gp_sgpr_fwd(x, xu, r, lengthscale.reshape(-1), variance.reshape(-1),
                                   None if alpha is None else alpha.reshape(-1), family)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gA, gb):
        from ... import kernels
        x, xu, r, lengthscale, variance, alpha = ctx.saved_tensors
        nx, nxu, nr, nl, nv, na = ctx.needs_input_grad[:6]
        gx, gxu, gl, gv, ga, gr = kernels.gp_sgpr_bwd(
            x, xu, r, lengthscale.reshape(-1), variance.reshape(-1), None if alpha is None else alpha.reshape(-1),
            gA, gb, ctx.family, (nx, nxu, nl, nv, na, nr))
        return (gx, gxu, gr, None if gl is None else gl.reshape(lengthscale.shape),
                None if gv is None else gv.reshape(variance.shape),
                None if ga is None else ga.reshape(alpha.shape), None)


class _ConditionalMarginals(torch.autograd.Function):
    """(loc [N, Q], s [N, 1 + Q]) = (Kuf^T a, |P_j Kuf[:, n]|^2) in one pass over x; the gradient is two more passes
    (weighted Grams for a and P, then the chain to x, xu and the kernel's parameters).  No double backward."""

    @staticmethod
    def forward(ctx, x, xu, a, P, lengthscale, variance, alpha, family):
        from ... import kernels
        ctx.family = family
        ctx.save_for_backward(x, xu, a, P, lengthscale, variance, alpha)
        return kernels.gp_cond_fwd(x, xu, a, P, lengthscale.reshape(-1), variance.reshape(-1),
                                   None if alpha is None else alpha.reshape(-1), family)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loc, g_s):
        from ... import kernels
        x, xu, a, P, lengthscale, variance, alpha = ctx.saved_tensors
        nx, nxu, na, nP, nl, nv, nal = ctx.needs_input_grad[:7]
        gx, gxu, gl, gv, gal, ga, gP = kernels.gp_cond_bwd(
            x, xu, a, P, lengthscale.reshape(-1), variance.reshape(-1), None if alpha is None else alpha.reshape(-1),
            g_loc, g_s, ctx.family, (nx, nxu, nl, nv, nal, na, nP))
        return (gx, gxu, ga, gP, None if gl is None else gl.reshape(lengthscale.shape),
                None if gv is None else gv.reshape(variance.shape),
                None if gal is None else gal.reshape(alpha.shape), None)


def conditional_factors(Luu, u_loc, u_scale_tril, whiten):
    """From q(u) = N(u_loc [Q, M], u_scale_tril [Q, M, M]) and the factor Luu of Kuu to what the streamed marginals
    need: a [M, Q] and P [1 + Q, M, M] with loc[q, n] = k_n . a_q, var[q, n] = clamp(kd_n - |P_0 k_n|^2, 0) +
    |P_{1+q} k_n|^2.  P_0 = Luu^-1; with ``whiten`` a = Luu^-T u_loc^T and P_{1+q} = S_q^T Luu^-1, else a = Kuu^-1 u_loc^T
    and P_{1+q} = (Luu^-1 S_q)^T Luu^-1."""
    M = Luu.size(0)
    Linv = torch.linalg.solve_triangular(Luu, torch.eye(M, dtype=Luu.dtype, device=Luu.device), upper=False)
    U = u_loc.t()
    if not whiten:
        U = torch.linalg.solve_triangular(Luu, U, upper=False)
        u_scale_tril = torch.linalg.solve_triangular(Luu, u_scale_tril, upper=False)
    a = torch.linalg.solve_triangular(Luu.t(), U, upper=True)
    return a, torch.cat((Linv.unsqueeze(0), u_scale_tril.transpose(-1, -2).matmul(Linv)))


def streamed_factors(Luu, A, b, noise):
    """From the statistics to the M x M quantities of the streamed route: C = Luu^-1 A Luu^-T, c = Luu^-1 b, and the
    factor LB of I + C / noise.  (W D^-1 W^T = C / noise and W D^-1 r = c / noise for W = Luu^-1 Kuf, D = noise I.)"""
    half = torch.linalg.solve_triangular(Luu, A, upper=False)
    C = torch.linalg.solve_triangular(Luu, half.t(), upper=False)      # (A is symmetric)
    c = torch.linalg.solve_triangular(Luu, b, upper=False)
    LB = torch.linalg.cholesky(_add_to_diagonal((C / noise).contiguous(), 1))
    return C, c, LB


def streamed_log_prob(Luu, A, b, rr, kd, noise, N, approx):
    """(log p(y), trace_term or None) of DTC / VFE from A = Kuf Kuf^T [M, M], b = Kuf r [M, Q], rr = sum r^2 and
    kd = sum_n k(x_n, x_n):  with v = LB^-1 c,
    log p(y) = -1/2 [Q (N log 2 pi + N log noise + 2 sum log diag LB) + rr / noise - |v|^2 / noise^2];
    VFE's trace_term = clamp((kd - tr C) / noise, min=0)."""
    Q = b.size(1)
    C, c, LB = streamed_factors(Luu, A, b, noise)
    v = torch.linalg.solve_triangular(LB, c, upper=False)
    logdet = N * (math.log(2 * math.pi) + noise.log()) + 2 * LB.diagonal().log().sum()
    log_prob = -0.5 * (Q * logdet + rr / noise - v.pow(2).sum() / noise ** 2)
    trace_term = ((kd - C.diagonal().sum()) / noise).clamp(min=0) if approx == "VFE" else None
    return log_prob, trace_term


class GPModel(Parameterized):
    """A GP prior f ~ GP(mean_function, kernel) over inputs X [N, ...] with outputs y [..., N] (or None)."""

    def __init__(self, X, y, kernel, mean_function=None, jitter=1e-6):
        assert isinstance(X, torch.Tensor), "X needs to be a torch Tensor instead of a {}".format(type(X))
        if y is not None:
            assert isinstance(y, torch.Tensor), "y needs to be a torch Tensor instead of a {}".format(type(y))
        super().__init__()
        self.set_data(X, y)
        self.kernel = kernel
        self.mean_function = mean_function if mean_function is not None else _zero_mean_function
        self.jitter = jitter

    def model(self):
        raise NotImplementedError

    def guide(self):
        raise NotImplementedError

    def forward(self, Xnew, full_cov=False):
        raise NotImplementedError

    def set_data(self, X, y=None):
        if y is not None and X.size(0) != y.size(-1):
            raise ValueError("Expected the number of input data points equal to the number of output data points, "
                             "but got {} and {}.".format(X.size(0), y.size(-1)))
        self.X = X
        self.y = y

    def _check_Xnew_shape(self, Xnew):
        if Xnew.dim() != self.X.dim():
            raise ValueError("Train data and test data should have the same number of dimensions, but got {} and {}."
                             .format(self.X.dim(), Xnew.dim()))
        if self.X.shape[1:] != Xnew.shape[1:]:
            raise ValueError("Train data and test data should have the same shape of features, but got {} and {}."
                             .format(self.X.shape[1:], Xnew.shape[1:]))

    def _observe(self, distribution):
        return primitives.sample(self._pyro_get_fullname("y"),
                                 distribution.expand_by(self.y.shape[:-1]).to_event(self.y.dim() - 1), obs=self.y)


class GPRegression(GPModel):
    """y = f(X) + eps, eps ~ N(0, noise): the marginal likelihood N(mean, K(X, X) + noise I) by a Cholesky factor."""

    def __init__(self, X, y, kernel, noise=None, mean_function=None, jitter=1e-6):
        super().__init__(X, y, kernel, mean_function, jitter)
        noise = self.X.new_tensor(1.0) if noise is None else noise
        self.noise = PyroParam(noise, constraints.positive)

    def _factor(self):
        Kff = self.kernel(self.X).contiguous()
        return torch.linalg.cholesky(_add_to_diagonal(Kff, self.jitter + self.noise))

    @pyro_method
    def model(self):
        self.set_mode("model")
        Lff = self._factor()
        f_loc = self.X.new_zeros(self.X.size(0)) + self.mean_function(self.X)
        if self.y is None:
            return f_loc, Lff.pow(2).sum(dim=-1)
        return self._observe(dist.MultivariateNormal(f_loc, scale_tril=Lff))

    @pyro_method
    def guide(self):
        self.set_mode("guide")
        self._load_pyro_samples()

    def forward(self, Xnew, full_cov=False, noiseless=True):
        """Mean and covariance (``full_cov``) or variance of the posterior of f(Xnew); with ``noiseless=False`` of
        y(Xnew).  Parameters are read from the guide."""
        self._check_Xnew_shape(Xnew)
        self.set_mode("guide")
        Lff = self._factor()
        residual = self.y - self.mean_function(self.X)
        loc, cov = conditional(Xnew, self.X, self.kernel, residual, None, Lff, full_cov, jitter=self.jitter)
        if not noiseless:
            if full_cov:
                M = Xnew.size(0)
                cov = cov.contiguous()
                cov.view(-1, M * M)[:, ::M + 1] += self.noise
            else:
                cov = cov + self.noise
        return loc + self.mean_function(Xnew), cov

    def iter_sample(self, noiseless=True):
        """A function ``sample(xnew)`` that draws y at one new point [1, ...] from the posterior and then conditions on
        its own draw, so that later queries may depend on earlier ones."""
        noise = self.noise.detach()
        N = self.X.size(0)
        state = {"X": self.X.clone().detach(), "y": self.y.clone().detach(), "N": N,
                 "Kff": _add_to_diagonal(self.kernel(self.X.detach()).contiguous(), noise)}

        def sample_next(xnew):
            if torch.isnan(xnew).any():
                raise ValueError("iter_sample: xnew has NaN entries")
            X, y, Kff, n = state["X"], state["y"], state["Kff"], state["N"]
            Lff = torch.linalg.cholesky(Kff)
            residual = y - self.mean_function(X)
            loc, var = conditional(xnew, X, self.kernel, residual, None, Lff, False, jitter=self.jitter)
            if not noiseless:
                var = var + noise
            ynew = torch.distributions.Normal(loc + self.mean_function(xnew), var.sqrt()).rsample()
            grown = Kff.new_empty(n + 1, n + 1)
            grown[:n, :n] = Kff
            cross = self.kernel(X, xnew).squeeze()
            grown[n, :n] = cross
            grown[:n, n] = cross
            grown[n, n] = self.kernel(xnew, xnew).squeeze() + self.jitter
            if grown.logdet() > -15.0:            # a (nearly) repeated point would make the matrix singular: skip it
                state.update(Kff=grown, N=n + 1, X=torch.cat((X, xnew)), y=torch.cat((y, ynew)))
            return ynew

        return sample_next


class SparseGPRegression(GPModel):
    """GP regression through M inducing inputs ``Xu`` [M, ...] (a parameter).  With W = (Luu^-1 Kuf)^T and
    Qff = W W^T, the marginal of y is N(mean, Qff + D) as a low-rank-plus-diagonal Gaussian:

    * "DTC":  D = noise;
    * "FITC": D = noise + diag(Kff - Qff);
    * "VFE" (default): D = noise, and the term -tr(Kff - Qff) / (2 noise) joins the log-density as a ``pyro.factor``.
    """

    def __init__(self, X, y, kernel, Xu, noise=None, mean_function=None, approx=None, jitter=1e-6):
        assert isinstance(Xu, torch.Tensor), "Xu needs to be a torch Tensor instead of a {}".format(type(Xu))
        super().__init__(X, y, kernel, mean_function, jitter)
        self.Xu = Parameter(Xu)
        noise = self.X.new_tensor(1.0) if noise is None else noise
        self.noise = PyroParam(noise, constraints.positive)
        if approx is None:
            approx = "VFE"
        if approx not in ("DTC", "FITC", "VFE"):
            raise ValueError("The sparse approximation method should be one of 'DTC', 'FITC', 'VFE'.")
        self.approx = approx

    def _inducing(self):
        """(Luu, Luu^-1 Kuf [M, N])."""
        Kuu = self.kernel(self.Xu).contiguous()
        Luu = torch.linalg.cholesky(_add_to_diagonal(Kuu, self.jitter))
        Kuf = self.kernel(self.Xu, self.X)
        return Luu, torch.linalg.solve_triangular(Luu, Kuf, upper=False)

    def _streamed(self):
        """(Luu, A, b, residual [N, Q], noise), all in FLOAT64, when the streamed route applies (module docstring), else
        None.  Float32 models are cast up here and run the float64 kernels and float64 M x M algebra: A rounded (or
        accumulated) in float32 is not a perturbation of Kuf, so Luu^-1 A Luu^-T would carry 2^-24 cond(Kuu) where the
        dense route's W W^T does not (at cond = 2e3 the loss was off by 14 times the dense float32 route's error)."""
        if not FUSED_SGPR or self.approx not in ("DTC", "VFE") or self.y is None or not isinstance(self.kernel, Isotropy):
            return None
        N, M = self.X.size(0), self.Xu.size(0)
        if N < max(FUSED_SGPR_MIN_N, 1) or M < 1 or self.y.dtype != self.X.dtype or self.y.device != self.X.device:
            return None
        fused = self.kernel._fused(self.Xu, self.X)
        if fused is None:
            return None
        from ... import kernels as hip
        Q = self.y.numel() // N
        if M > hip.GP_SGPR_MAX_M[torch.float64] or not 1 <= Q <= hip.GP_SGPR_MAX_Q or not self.noise.is_cuda:
            return None
        xu, x, lengthscale, variance, alpha = (None if t is None else t.double() for t in fused)
        Kuu = self.kernel(self.Xu).contiguous().double()
        Luu = torch.linalg.cholesky(_add_to_diagonal(Kuu, self.jitter))
        residual = (self.y - self.mean_function(self.X)).reshape(-1, N).t().contiguous().double()
        A, b = _StreamedStatistics.apply(x, xu, residual, lengthscale, variance, alpha, self.kernel._family)
        return Luu, A, b, residual, self.noise.double()

    @pyro_method
    def model(self):
        self.set_mode("model")
        N = self.X.size(0)
        streamed = self._streamed()
        if streamed is not None:
            Luu, A, b, residual, noise = streamed
            kd = self.kernel(self.X, diag=True).double().sum()
            log_prob, trace_term = streamed_log_prob(Luu, A, b, residual.pow(2).sum(), kd, noise, N, self.approx)
            if trace_term is not None:
                primitives.factor(self._pyro_get_fullname("trace_term"), (-trace_term / 2.0).to(self.X.dtype))
            primitives.factor(self._pyro_get_fullname("y"), log_prob.to(self.X.dtype))
            return self.y
        _, Wt = self._inducing()
        W = Wt.t()
        D = self.noise.expand(N)
        trace_term = None
        if self.approx in ("FITC", "VFE"):
            residual_diag = self.kernel(self.X, diag=True) - W.pow(2).sum(dim=-1)
            if self.approx == "FITC":
                D = D + residual_diag
            else:
                trace_term = (residual_diag.sum() / self.noise).clamp(min=0)
        f_loc = self.X.new_zeros(N) + self.mean_function(self.X)
        if self.y is None:
            return f_loc, D + W.pow(2).sum(dim=-1)
        if trace_term is not None:
            primitives.factor(self._pyro_get_fullname("trace_term"), -trace_term / 2.0)
        return self._observe(dist.LowRankMultivariateNormal(f_loc, W, D))

    @pyro_method
    def guide(self):
        self.set_mode("guide")
        self._load_pyro_samples()

    def forward(self, Xnew, full_cov=False, noiseless=True):
        """Mean and covariance (``full_cov``) or variance of the posterior of f(Xnew) (of y(Xnew) with
        ``noiseless=False``).  With Ws = Luu^-1 Kus and L L^T = I + W D^-1 W^T (W = Luu^-1 Kuf):
        loc = (L^-1 Ws)^T L^-1 W D^-1 y,  cov = Kss - Ws^T Ws + (L^-1 Ws)^T (L^-1 Ws)."""
        self._check_Xnew_shape(Xnew)
        self.set_mode("guide")
        N = self.X.size(0)
        streamed = self._streamed()
        if streamed is not None:          # W D^-1 W^T = C / noise and W D^-1 y = c / noise, from the statistics
            Luu, A, b, _, noise = streamed
            _, c, L = streamed_factors(Luu, A, b, noise)
            Luu, L, W_Dinv_y = Luu.to(self.X.dtype), L.to(self.X.dtype), (c / noise).to(self.X.dtype)
        else:
            Luu, W = self._inducing()
            D = self.noise.expand(N)
            if self.approx == "FITC":
                D = D + self.kernel(self.X, diag=True) - W.pow(2).sum(dim=0)
            W_Dinv = W / D
            L = torch.linalg.cholesky(_add_to_diagonal(W_Dinv.matmul(W.t()).contiguous(), 1))
            residual = (self.y - self.mean_function(self.X)).reshape(-1, N).t()
            W_Dinv_y = W_Dinv.matmul(residual)
        n_out = W_Dinv_y.size(1)
        Ws = torch.linalg.solve_triangular(Luu, self.kernel(self.Xu, Xnew), upper=False)
        solved = torch.linalg.solve_triangular(L, torch.cat((W_Dinv_y, Ws), dim=1), upper=False)
        Linv_W_Dinv_y, Linv_Ws = solved[:, :n_out], solved[:, n_out:]
        C = Xnew.size(0)
        batch = self.y.shape[:-1]
        loc = Linv_W_Dinv_y.t().matmul(Linv_Ws).reshape(batch + (C,))
        if full_cov:
            Kss = self.kernel(Xnew).contiguous()
            if not noiseless:
                _add_to_diagonal(Kss, self.noise)
            cov = (Kss - Ws.t().matmul(Ws) + Linv_Ws.t().matmul(Linv_Ws)).expand(batch + (C, C))
        else:
            Kss_diag = self.kernel(Xnew, diag=True)
            if not noiseless:
                Kss_diag = Kss_diag + self.noise
            cov = (Kss_diag - Ws.pow(2).sum(dim=0) + Linv_Ws.pow(2).sum(dim=0)).expand(batch + (C,))
        return loc + self.mean_function(Xnew), cov


class VariationalSparseGP(GPModel):
    """A sparse GP with a variational posterior q(u) = N(u_loc, u_scale_tril u_scale_tril^T) over the values at M
    inducing inputs ``Xu`` [M, ...] (a parameter) and any ``likelihood``; trainable on mini-batches (``set_data`` with
    ``num_data`` the size of the whole data set).  ``latent_shape`` is the batch shape of the latent functions (y's by
    default); with ``whiten`` q describes v = Luu^-1 u instead."""

    def __init__(self, X, y, kernel, Xu, likelihood, mean_function=None, latent_shape=None, num_data=None, whiten=False,
                 jitter=1e-6):
        assert isinstance(Xu, torch.Tensor), "Xu needs to be a torch Tensor instead of a {}".format(type(Xu))
        super().__init__(X, y, kernel, mean_function, jitter)
        self.likelihood = likelihood
        self.Xu = Parameter(Xu)
        y_batch_shape = self.y.shape[:-1] if self.y is not None else torch.Size([])
        self.latent_shape = torch.Size(latent_shape) if latent_shape is not None else y_batch_shape
        M = self.Xu.size(0)
        self.u_loc = Parameter(self.Xu.new_zeros(self.latent_shape + (M,)))
        identity = torch.eye(M, dtype=self.Xu.dtype, device=self.Xu.device)
        self.u_scale_tril = PyroParam(identity.repeat(self.latent_shape + (1, 1)), constraints.lower_cholesky)
        self.num_data = num_data if num_data is not None else self.X.size(0)
        self.whiten = whiten

    def _factor(self):
        Kuu = self.kernel(self.Xu).contiguous()
        return torch.linalg.cholesky(_add_to_diagonal(Kuu, self.jitter))

    def _streamed(self, X, Luu):
        """(loc, var) of f(X), each ``latent_shape + (N,)``, by the streamed route when it applies (module docstring), else
        None.  Float64 models only: a float32 model cast up to the float64 kernels (Luu still factored in float32) missed
        four times the dense float32 route's own error in three of the device test's eight cases (by 1.3, 1.6 and 5.0
        times), so float32 models stay on the dense route."""
        if not FUSED_VSGP or not isinstance(self.kernel, Isotropy):
            return None
        N, M, Q = X.size(0), self.Xu.size(0), self.latent_shape.numel()
        if N < max(FUSED_VSGP_MIN_N, 1) or M < 1 or X.dtype != torch.float64:
            return None
        fused = self.kernel._fused(self.Xu, X)
        from ... import kernels as hip
        if fused is None or M > hip.GP_COND_MAX_M[torch.float64] or not 1 <= Q <= hip.GP_COND_MAX_Q:
            return None
        if not (self.u_loc.is_cuda and self.u_loc.dtype == X.dtype):
            return None
        xu, x, lengthscale, variance, alpha = fused
        a, P = conditional_factors(Luu, self.u_loc.reshape(Q, M), self.u_scale_tril.reshape(Q, M, M), self.whiten)
        loc, s = _ConditionalMarginals.apply(x, xu, a, P, lengthscale, variance, alpha, self.kernel._family)
        var = (self.kernel(X, diag=True) - s[:, 0]).clamp(min=0) + s[:, 1:].t()
        shape = self.latent_shape + (N,)
        return loc.t().reshape(shape), var.reshape(shape)

    def _marginals(self, X, Luu):
        streamed = self._streamed(X, Luu)
        if streamed is not None:
            return streamed
        return util.conditional(X, self.Xu, self.kernel, self.u_loc, self.u_scale_tril, Luu, full_cov=False,
                                whiten=self.whiten, jitter=self.jitter)

    @pyro_method
    def model(self):
        self.set_mode("model")
        Luu = self._factor()
        zero_loc = self.Xu.new_zeros(self.u_loc.shape)
        prior_tril = torch.eye(Luu.size(0), dtype=Luu.dtype, device=Luu.device) if self.whiten else Luu
        primitives.sample(self._pyro_get_fullname("u"),
                          dist.MultivariateNormal(zero_loc, scale_tril=prior_tril).to_event(zero_loc.dim() - 1))
        f_loc, f_var = self._marginals(self.X, Luu)
        f_loc = f_loc + self.mean_function(self.X)
        if self.y is None:
            return f_loc, f_var
        self.likelihood._load_pyro_samples()      # (the likelihood's own priors are not scaled)
        with poutine.scale(scale=self.num_data / self.X.size(0)):
            return self.likelihood(f_loc, f_var, self.y)

    @pyro_method
    def guide(self):
        self.set_mode("guide")
        self._load_pyro_samples()
        primitives.sample(self._pyro_get_fullname("u"),
                          dist.MultivariateNormal(self.u_loc, scale_tril=self.u_scale_tril).to_event(self.u_loc.dim() - 1))

    def forward(self, Xnew, full_cov=False):
        """Mean and covariance (``full_cov``) or variance of the posterior of f(Xnew); parameters are read from the
        guide."""
        self._check_Xnew_shape(Xnew)
        self.set_mode("guide")
        if full_cov:
            loc, cov = util.conditional(Xnew, self.Xu, self.kernel, self.u_loc, self.u_scale_tril, full_cov=True,
                                        whiten=self.whiten, jitter=self.jitter)
        else:
            loc, cov = self._marginals(Xnew, self._factor())
        return loc + self.mean_function(Xnew), cov
