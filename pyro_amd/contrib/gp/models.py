"""Gaussian-process regression models (the classes and arguments of pyro/contrib/gp/models; the code is this
package's): ``GPModel``, exact ``GPRegression`` and ``SparseGPRegression`` with the DTC, FITC and VFE approximations.

A model closes over its data: ``model()`` and ``guide()`` take no arguments, so an SVI step over them is eager (see
``util.train``).  Covariance matrices come from ``self.kernel``; on the device the stationary families form them in one
launch (``kernels.FUSED_GP_KERNEL``).  Noise and jitter are added to the diagonal of the matrix IN PLACE, as the
reference does; the fused kernel's backward recomputes what it needs from the inputs, so that is allowed.
"""
import torch
from torch.distributions import constraints
from torch.nn import Parameter

from ... import distributions as dist
from ... import primitives
from ...nn.module import PyroParam, pyro_method
from .parameterized import Parameterized
from .util import conditional


def _zero_mean_function(x):
    return 0


def _add_to_diagonal(matrix, value):
    """matrix [n, n] (contiguous) += value * I, in place; returns it."""
    n = matrix.size(-1)
    matrix.view(-1)[::n + 1] += value
    return matrix


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

    @pyro_method
    def model(self):
        self.set_mode("model")
        N = self.X.size(0)
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
        M = self.Xu.size(0)
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
