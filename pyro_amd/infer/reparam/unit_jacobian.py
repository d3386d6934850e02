"""Reparameterisers through a transform whose Jacobian determinant is one (role of pyro/infer/reparam/
{unit_jacobian,haar,discrete_cosine}.py): a time-local latent -- a drift, a seasonal innovation -- is sampled in a
wavelet or frequency basis, where a random walk's coordinates are nearly independent, so that neither NUTS nor a
mean-field guide has to fight their correlations.  On device tensors each direction of the transform is one launch of
pa_time_transform (pyro_amd.ops.tensor_utils), and its gradient one more."""
from contextlib import ExitStack

from torch.distributions import biject_to
from torch.distributions.transforms import ComposeTransform

from ...distributions.transforms import DiscreteCosineTransform, HaarTransform
from ...poutine.plate_messenger import block_plate
from .reparam import Reparam


class UnitJacobianReparam(Reparam):
    """The auxiliary site ``<name>_<suffix>`` is ``TransformedDistribution(fn, [biject_to(fn.support).inv,
    transform])``; the site itself becomes a Delta at the back-transformed value.

    ``experimental_allow_batch``: a transform that reaches into the batch dims of the site (a time plate's dim, most
    often) is allowed; the targeted batch dim and those to its right become event dims (contrib.forecast.util.
    reshape_batch) and their plates are muted while the auxiliary site is drawn (poutine.block_plate).  Without it
    such a transform raises ValueError."""

    def __init__(self, transform, suffix="transformed", *, experimental_allow_batch=False):
        self.transform = transform.with_cache()
        self.suffix = suffix
        self.experimental_allow_batch = experimental_allow_batch

    def apply(self, msg):
        from ... import distributions as dist
        from ...primitives import sample
        fn, value = msg["fn"], msg["value"]
        event_dim = fn.event_dim
        transform = self.transform
        shift = max(0, transform.domain.event_dim - event_dim)
        with ExitStack() as stack:
            if shift:
                if not self.experimental_allow_batch:
                    raise ValueError("Cannot transform along batch dimension; try either converting a batch dimension "
                                     "to an event dimension, or setting experimental_allow_batch=True.")
                from ...contrib.forecast.util import reshape_batch, reshape_transform_batch
                old = tuple(fn.batch_shape)
                if len(old) < shift:
                    raise ValueError("the transform reaches {} dims into a batch shape of {}".format(shift, old))
                new = old[:-shift] + (1,) * shift + old[-shift:]
                tail = tuple(fn.event_shape)
                fn = reshape_batch(fn, new).to_event(shift)
                transform = reshape_transform_batch(transform, old + tail, new + tail)
                if value is not None:
                    cut = value.dim() - shift - event_dim
                    value = value.reshape(value.shape[:cut] + (1,) * shift + value.shape[cut:])
                for dim in range(-shift, 0):
                    stack.enter_context(block_plate(dim=dim, strict=False))
            chain = ComposeTransform([biject_to(fn.support).inv.with_cache(), transform])
            known = None if value is None else chain(value)
            aux = sample("{}_{}".format(msg["name"], self.suffix), dist.TransformedDistribution(fn, chain), obs=known,
                         infer={"is_observed": msg["is_observed"]})
        if value is None:
            value = chain.inv(aux)
        if shift:
            cut = value.dim() - 2 * shift - event_dim
            value = value.reshape(value.shape[:cut] + value.shape[cut + shift:])
        return {"fn": dist.Delta(value, event_dim=event_dim).mask(False), "value": value, "is_observed": True}


class HaarReparam(UnitJacobianReparam):
    """The site ``<name>_haar`` holds the Haar wavelet coefficients along ``dim`` (negative, absolute); ``flip``:
    reverse time first, so that the short blocks of a length that is no power of two come first in time."""

    def __init__(self, dim=-1, flip=False, *, experimental_allow_batch=False):
        super().__init__(HaarTransform(dim=dim, flip=flip, cache_size=1), suffix="haar",
                         experimental_allow_batch=experimental_allow_batch)


class DiscreteCosineReparam(UnitJacobianReparam):
    """The site ``<name>_dct`` holds the orthonormal DCT-II coefficients along ``dim`` (negative, absolute), frequency
    k + 1/2 weighted by (k + 1/2) ** smooth (0: white noise stays white; 1: Brownian noise becomes white)."""

    def __init__(self, dim=-1, smooth=0.0, *, experimental_allow_batch=False):
        super().__init__(DiscreteCosineTransform(dim=dim, smooth=smooth, cache_size=1), suffix="dct",
                         experimental_allow_batch=experimental_allow_batch)
