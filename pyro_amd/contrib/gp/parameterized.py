"""``Parameterized``: a ``PyroModule`` whose attributes can be given priors, each with a guide of its own (the role of
pyro/contrib/gp/parameterized.py; parameter names as the reference's, so checkpoints carry over).

* ``module.attr = PyroSample(prior)`` records the prior and installs a point-mass guide, the parameter ``attr_map``;
* ``module.autoguide("attr", dist.Normal)`` replaces it by a diagonal Normal (``attr_loc``, ``attr_scale``), and
  ``dist.MultivariateNormal`` by a full one (``attr_loc``, ``attr_scale_tril``); the parameters of the guide that is
  replaced are deleted;
* ``module.set_mode("model" | "guide")`` decides, for this module and every ``Parameterized`` below it, whether
  reading ``module.attr`` draws from the prior or from the guide.

A Normal guide of a prior whose support is not the real line lives in unconstrained space: the guide draws the
auxiliary site ``<attr>_latent`` there and ``attr`` itself is a point mass at the transformed draw, carrying the
log-Jacobian of the transform.
"""
import collections
import functools
import warnings

import torch
from torch.distributions import biject_to, constraints

from ... import distributions as dist
from ... import primitives
from ...nn.module import PyroModule, PyroParam, PyroSample, pyro_method

_GUIDES = {"Delta": ("map",), "Normal": ("loc", "scale"), "MultivariateNormal": ("loc", "scale_tril")}


def _real_support(support):
    while isinstance(support, constraints.independent):
        support = support.base_constraint
    return support is constraints.real or support is constraints.real_vector


def _site_distribution(module, name):
    """What ``module.<name>`` is sampled from in the module's present mode."""
    prior = module._priors[name]
    if module.mode == "model":
        return prior
    kind, fields = module._guides[name]
    if kind == "Delta":
        point = getattr(module, name + "_map")
        return dist.Delta(point, event_dim=point.dim())
    guide = getattr(dist, kind)(**{f: getattr(module, "{}_{}".format(name, f)) for f in fields})
    guide = guide.to_event()
    if _real_support(prior.support):
        return guide
    latent = primitives.sample(module._pyro_get_fullname(name + "_latent"), guide, infer={"is_auxiliary": True})
    transform = biject_to(prior.support)
    value = transform(latent)
    log_density = transform.inv.log_abs_det_jacobian(value, latent).sum()
    return dist.Delta(value, log_density, event_dim=value.dim())


class Parameterized(PyroModule):
    def __init__(self):
        super().__init__()
        self._priors = collections.OrderedDict()
        self._guides = collections.OrderedDict()
        self._mode = "model"

    def _pyro_get_fullname(self, name):
        """The dotted name of attribute ``name`` in the module tree this module was attached to."""
        prefix = self.__dict__.get("_pyro_name", "")
        return "{}.{}".format(prefix, name) if prefix else name

    def __setattr__(self, name, value):
        if isinstance(value, PyroSample) and hasattr(value.prior, "sample"):
            self._priors[name] = value.prior
            self.autoguide(name, dist.Delta)
            value = PyroSample(functools.partial(_site_distribution, name=name))
        super().__setattr__(name, value)

    def set_prior(self, name, prior):
        warnings.warn("set_prior({0!r}, prior) is deprecated: assign module.{0} = PyroSample(prior)".format(name),
                      UserWarning)
        setattr(self, name, PyroSample(prior))

    def autoguide(self, name, dist_constructor):
        """The guide of attribute ``name`` (which must have a prior): ``dist.Delta``, ``dist.Normal`` or
        ``dist.MultivariateNormal``, initialised at a draw of the prior."""
        if name not in self._priors:
            raise ValueError("There is no prior for parameter: {}".format(name))
        kind = getattr(dist_constructor, "__name__", None)
        if kind not in _GUIDES or dist_constructor is not getattr(dist, kind):
            raise NotImplementedError("Unsupported distribution type: {}".format(dist_constructor))
        if name in self._guides:
            for field in self._guides[name][1]:
                delattr(self, "{}_{}".format(name, field))
        prior = self._priors[name]
        with torch.no_grad():
            draw = prior().detach()
        if kind == "Delta":
            if _real_support(prior.support):
                setattr(self, name + "_map", torch.nn.Parameter(draw))
            else:
                setattr(self, name + "_map", PyroParam(draw, prior.support))
        else:
            loc = biject_to(prior.support).inv(draw).detach()
            setattr(self, name + "_loc", torch.nn.Parameter(loc))
            if kind == "Normal":
                setattr(self, name + "_scale", PyroParam(torch.ones_like(loc), constraints.positive))
            else:
                n = loc.size(-1)
                eye = torch.eye(n, dtype=loc.dtype, device=loc.device)
                setattr(self, name + "_scale_tril",
                        PyroParam(eye.repeat(loc.shape[:-1] + (1, 1)), constraints.lower_cholesky))
        self._guides[name] = (kind, _GUIDES[kind])

    @pyro_method
    def _load_pyro_samples(self):
        """Read (and thereby sample) every attribute with a prior, in this module and below it."""
        for module in self.modules():
            for name in list(module.__dict__.get("_pyro_samples", ())):
                getattr(module, name)

    def set_mode(self, mode):
        for module in self.modules():
            if isinstance(module, Parameterized):
                module.mode = mode

    @property
    def mode(self):
        return self._mode

    @mode.setter
    def mode(self, mode):
        self._mode = mode
