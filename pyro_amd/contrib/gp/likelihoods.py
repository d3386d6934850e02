"""Likelihoods of variational GP models (the classes, arguments and site names of pyro/contrib/gp/likelihoods; the
code is this package's): given the marginals of the latent function, ``f_loc`` and ``f_var`` of shape
``latent_shape + (N,)``, a likelihood observes ``y`` at the site ``y``.

``Gaussian`` integrates f out in closed form; the others draw ONE f from the marginals (a one-sample Monte-Carlo
estimate of the expected log-likelihood) and map it through ``response_function`` into the parameter of the observation
distribution.  The default response functions go through ``logits``, which is stable for large |f|.
"""
import torch
from torch.distributions import constraints

from ... import distributions as dist
from ... import primitives
from ...nn.module import PyroParam
from .parameterized import Parameterized


def _draw(f_loc, f_var):
    """One reparameterised draw of Normal(f_loc, sqrt(f_var)); a variance clamped to exactly 0 gives f_loc."""
    return f_loc + f_var.sqrt() * torch.randn_like(f_loc)


def _softmax(x):
    return torch.softmax(x, dim=-1)


class Likelihood(Parameterized):
    """p(y | f) for the latent function values f ~ N(f_loc, f_var)."""

    def forward(self, f_loc, f_var, y=None):
        raise NotImplementedError

    def _observe(self, y_dist, y, latent_dims):
        """The site ``y``: ``y_dist`` (whose batch shape is y's last ``latent_dims`` dimensions) expanded to y."""
        if y is not None:
            y_dist = y_dist.expand_by(y.shape[:y.dim() - latent_dims]).to_event(y.dim())
        return primitives.sample(self._pyro_get_fullname("y"), y_dist, obs=y)


class Gaussian(Likelihood):
    """y ~ Normal(f_loc, sqrt(f_var + variance)): regression with the noise ``variance`` (a positive parameter)."""

    def __init__(self, variance=None):
        super().__init__()
        variance = torch.tensor(1.0) if variance is None else variance
        self.variance = PyroParam(variance, constraints.positive)

    def forward(self, f_loc, f_var, y=None):
        return self._observe(dist.Normal(f_loc, (f_var + self.variance).sqrt()), y, f_loc.dim())


class Binary(Likelihood):
    """y ~ Bernoulli(response_function(f)), f ~ Normal(f_loc, sqrt(f_var)); the response is the sigmoid by default."""

    def __init__(self, response_function=None):
        super().__init__()
        self.response_function = torch.sigmoid if response_function is None else response_function

    def forward(self, f_loc, f_var, y=None):
        f = _draw(f_loc, f_var)
        if self.response_function is torch.sigmoid:
            y_dist = dist.Bernoulli(logits=f)
        else:
            y_dist = dist.Bernoulli(self.response_function(f))
        return self._observe(y_dist, y, f.dim())


class Poisson(Likelihood):
    """y ~ Poisson(response_function(f)), f ~ Normal(f_loc, sqrt(f_var)); the response is exp by default."""

    def __init__(self, response_function=None):
        super().__init__()
        self.response_function = torch.exp if response_function is None else response_function

    def forward(self, f_loc, f_var, y=None):
        f = _draw(f_loc, f_var)
        return self._observe(dist.Poisson(self.response_function(f)), y, f.dim())


class MultiClass(Likelihood):
    """y ~ Categorical(response_function(f^T)) over ``num_classes`` classes, one latent function per class:
    f ~ Normal(f_loc, sqrt(f_var)) is [..., num_classes, N] and y [..., N] holds class indices.  The response
    normalises the last axis; it is the softmax by default."""

    def __init__(self, num_classes, response_function=None):
        super().__init__()
        self.num_classes = num_classes
        self.response_function = _softmax if response_function is None else response_function

    def forward(self, f_loc, f_var, y=None):
        f = _draw(f_loc, f_var)
        if f.dim() < 2:
            raise ValueError("Latent function output should have at least 2 dimensions: one for number of classes and "
                             "one for number of data.")
        f_swap = f.transpose(-2, -1)                     # [..., N, num_classes]
        if f_swap.size(-1) != self.num_classes:
            raise ValueError("Number of Gaussian processes should be equal to the number of classes. Expected {} but "
                             "got {}.".format(self.num_classes, f_swap.size(-1)))
        if self.response_function is _softmax:
            y_dist = dist.Categorical(logits=f_swap)
        else:
            y_dist = dist.Categorical(self.response_function(f_swap))
        return self._observe(y_dist, y, f.dim() - 1)
