"""Auxiliary-variable reparameteriser of StudentT sites (role of pyro/infer/reparam/studentt.py): a Student-t
variable is a Normal whose precision is scaled by a Gamma(df / 2, df / 2) draw.  With ``LinearHMMReparam`` it makes a
heavy-tailed linear state-space model conditionally Gaussian, so that its likelihood is one ``GaussianHMM``."""
import torch

from ... import distributions as dist
from ...primitives import sample
from .reparam import Reparam


class StudentTReparam(Reparam):
    """The auxiliary site is ``<name>_gamma ~ Gamma(df / 2, df / 2)`` with the site's event dims; the site itself
    becomes ``Normal(loc, scale * gamma.rsqrt())``, its value and observedness unchanged."""

    def apply(self, msg):
        fn, event_dim = self._unwrap(msg["fn"])
        assert isinstance(fn, torch.distributions.StudentT), type(fn).__name__
        half_df = fn.df * 0.5
        gamma = sample("{}_gamma".format(msg["name"]), self._wrap(dist.Gamma(half_df, half_df), event_dim))
        new_fn = self._wrap(dist.Normal(fn.loc, fn.scale * gamma.rsqrt()), event_dim)
        return {"fn": new_fn, "value": msg["value"], "is_observed": msg["is_observed"]}
