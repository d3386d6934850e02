"""Reparameterisers (reference: pyro/infer/reparam/{reparam,loc_scale,transform,studentt,hmm}.py) for
``poutine.reparam``: a sample site is replaced by an auxiliary site in better-conditioned coordinates
followed by a deterministic map back -- the usual cure for funnel-shaped posteriors under HMC / NUTS and
mean-field guides -- or by auxiliary sites conditioned on which it has a tractable density.  Provided: non-centring
of location-scale families, sampling the base of a TransformedDistribution, the StudentT route from a LinearHMM
to a conditionally Gaussian GaussianHMM, and sampling a time-local latent in a Haar or DCT basis (unit_jacobian.py)."""
from .unit_jacobian import DiscreteCosineReparam, HaarReparam, UnitJacobianReparam  # noqa: F401
from .hmm import LinearHMMReparam  # noqa: F401
from .loc_scale import LocScaleReparam  # noqa: F401
from .reparam import Reparam  # noqa: F401
from .studentt import StudentTReparam  # noqa: F401
from .transform import TransformReparam  # noqa: F401
