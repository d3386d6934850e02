"""What ``ForecastingModel.predict`` and ``Forecaster.__call__`` need around the noise distribution: two handlers and
three single-dispatch functions over distribution types (the public names are those of the reference's
pyro.contrib.forecast.util; the code is this package's).

``reshape_batch(d, batch_shape)``: ``d`` with another batch shape of the same number of elements -- ``predict`` uses
it to move the time batch dim of a noise distribution out of the way, ``batch_shape + (1,)``.
``prefix_condition(d, data)``: ``d`` over ``batch + (t + f, obs)`` given its first ``t`` steps -> ``batch + (f, obs)``.
``reshape_transform_batch(t, old_shape, new_shape)``: an element-wise transform whose parameters follow its base
distribution from ``old_shape`` to ``new_shape`` (the DCT and Haar transforms count their dim from the right and stay).
``time_reparam_dct(msg)``, ``time_reparam_haar(msg)``: configs for ``poutine.reparam`` that sample every unobserved
site inside the time plate in a frequency or wavelet basis.

How it is organised.  A distribution that is nothing but tensors of its own shape is described ONCE, in TENSOR_FAMILIES:
class -> ((constructor keyword, event rank of that tensor), ...).  Both operations are then one function applied to
every such tensor (``_each_tensor``): reshaping expands a tensor to the distribution's batch and views it under the
new one; conditioning on a prefix cuts the time axis, which is the second-to-last dim of the distribution's full shape
wherever that falls in the tensor (``_time_axis``).  The element-wise families and MultivariateNormal are rows of that
table; Independent, MaskedDistribution, TransformedDistribution and IndependentHMM pass the operation on to what they
wrap; the two HMM classes have code of their own.

GaussianHMM keeps its parameters SHARED: when the new batch shape only adds or drops size-1 dims -- what ``predict``
asks for -- every part is a view of the old one with the same size-1 dims added or dropped, so a stride-0 (expanded)
or time-homogeneous parameter stays one and still reaches the Kalman kernel as one matrix for all sequences.  (The
reference expands every part to the full batch first.)  Any other reshape expands the parts that differ between
sequences and leaves a part that all sequences share as it is.
"""
from functools import singledispatch

import torch
from torch.distributions import transforms

from ... import distributions as dist
from ...poutine.runtime import Messenger
from ...poutine.util import site_is_subsample


# ---- the two handlers ------------------------------------------------------------------------------------------------
class PrefixReplayMessenger(Messenger):
    """Runs a model over MORE time steps than the guide trace it is given covers.  A site of the trace keeps the
    trace's value; where the model's value is longer along one axis (time), the trace's value is written over the
    beginning of the model's own draw, whose remainder -- a draw from the prior -- stays."""

    def __init__(self, trace):
        super().__init__()
        self.trace = trace

    def _pyro_post_sample(self, msg):
        name = msg["name"]
        if name not in self.trace.nodes or site_is_subsample(msg):
            return
        drawn, known = msg["value"], self.trace.nodes[name]["value"]
        if drawn.shape != known.shape:
            longer = [axis for axis in range(min(drawn.dim(), known.dim())) if drawn.size(axis) != known.size(axis)]
            if drawn.dim() != known.dim() or len(longer) != 1 or drawn.size(longer[0]) < known.size(longer[0]):
                raise ValueError("site {!r}: the model's value {} does not extend the trace's {} along one axis"
                                 .format(name, tuple(drawn.shape), tuple(known.shape)))
            axis = longer[0]
            known = torch.cat([known, drawn.narrow(axis, known.size(axis), drawn.size(axis) - known.size(axis))], axis)
        msg["value"] = known


class PrefixConditionMessenger(Messenger):
    """``data``: {site name: its first observations [..., t, obs]}.  A named site that is about to be sampled gets,
    in place of its distribution, that distribution given the observations (``prefix_condition``)."""

    def __init__(self, data):
        super().__init__()
        self.data = data

    def _pyro_sample(self, msg):
        observed = self.data.get(msg["name"])
        if observed is None:
            return
        if msg["value"] is not None:
            raise RuntimeError("site {!r} already has a value: nothing is left to forecast".format(msg["name"]))
        msg["fn"] = prefix_condition(msg["fn"], observed)


# ---- configs for poutine.reparam -------------------------------------------------------------------------------------
def _time_reparam(msg, make):
    if msg["is_observed"] or site_is_subsample(msg):
        return None
    for frame in msg["cond_indep_stack"]:
        if frame.name == "time":
            return make(dim=frame.dim - msg["fn"].event_dim, experimental_allow_batch=True)
    return None


def time_reparam_dct(msg):
    """A config for ``poutine.reparam``: every unobserved site inside the plate named ``"time"`` is sampled as its
    DCT coefficients along time (a ``DiscreteCosineReparam`` along ``frame.dim - fn.event_dim``).  The reference's
    function of this name returns a HaarReparam and its ``time_reparam_haar`` a DiscreteCosineReparam; that slip is
    not copied here."""
    from ...infer.reparam import DiscreteCosineReparam
    return _time_reparam(msg, DiscreteCosineReparam)


def time_reparam_haar(msg):
    """A config for ``poutine.reparam``: every unobserved site inside the plate named ``"time"`` is sampled as its
    Haar wavelet coefficients along time (a ``HaarReparam`` along ``frame.dim - fn.event_dim``).  The reference's
    function of this name returns a DiscreteCosineReparam and its ``time_reparam_dct`` a HaarReparam; that slip is
    not copied here."""
    from ...infer.reparam import HaarReparam
    return _time_reparam(msg, HaarReparam)


# ---- distributions that are tensors of their own shape ---------------------------------------------------------------
def _elementwise(*names):
    return tuple((name, 0) for name in names)


# class -> ((constructor keyword, event rank of that tensor), ...)
TENSOR_FAMILIES = {
    dist.Normal: _elementwise("loc", "scale"),
    dist.StudentT: _elementwise("df", "loc", "scale"),
    dist.Laplace: _elementwise("loc", "scale"),
    dist.Cauchy: _elementwise("loc", "scale"),
    dist.LogNormal: _elementwise("loc", "scale"),
    dist.Gamma: _elementwise("concentration", "rate"),
    dist.Exponential: _elementwise("rate"),
    dist.Poisson: _elementwise("rate"),
    dist.Bernoulli: _elementwise("logits"),
    dist.Beta: _elementwise("concentration1", "concentration0"),
    dist.Uniform: _elementwise("low", "high"),
    dist.MultivariateNormal: (("loc", 1), ("scale_tril", 2)),
}
# element-wise transform class -> the names of its tensor-or-number parameters
ELEMENTWISE_TRANSFORMS = {
    transforms.AffineTransform: ("loc", "scale"),
    transforms.PowerTransform: ("exponent",),
    transforms.ExpTransform: (),
    transforms.SigmoidTransform: (),
    transforms.AbsTransform: (),
}


def _each_tensor(d, change):
    """A distribution of ``d``'s class from ``change(tensor, rank)`` of each of its tensors."""
    return type(d)(**{name: change(getattr(d, name), rank) for name, rank in TENSOR_FAMILIES[type(d)]},
                   validate_args=d.__dict__.get("_validate_args"))


def _time_axis(d, rank):
    """Where time sits in a tensor of event rank ``rank`` of ``d``: time is the second-to-last dim of batch + event."""
    return -(2 - len(d.event_shape) + rank)


def _unsupported(what, thing):
    return NotImplementedError("{} has no rule for {}".format(what, type(thing).__name__))


# ---- prefix_condition ------------------------------------------------------------------------------------------------
@singledispatch
def prefix_condition(d, data):
    """``d`` over ``batch + (t + f, obs)`` given ``data`` [..., t, obs], its first ``t`` steps: the distribution of
    the other ``f`` steps.  A class outside this module takes part by having a method of this name."""
    own = getattr(d, "prefix_condition", None)
    if own is None:
        raise _unsupported("prefix_condition()", d)
    return own(data)


def _drop_observed_steps(d, data):
    # the steps are independent given the parameters: what remains is the parameters' tail
    seen = data.size(-2)
    return _each_tensor(d, lambda v, rank: v.narrow(_time_axis(d, rank), seen, v.size(_time_axis(d, rank)) - seen))


@prefix_condition.register(torch.distributions.Independent)
def _(d, data):
    return prefix_condition(d.base_dist, data).to_event(d.reinterpreted_batch_ndims)


@prefix_condition.register(dist.MaskedDistribution)
def _(d, data):
    rest = prefix_condition(d.base_dist, data)
    keep = d._mask
    if isinstance(keep, torch.Tensor):
        axis = _time_axis(d, 0)                    # (the mask has the batch shape)
        keep = keep.narrow(axis, data.size(-2), keep.size(axis) - data.size(-2))
    return rest.mask(keep)


@prefix_condition.register(torch.distributions.TransformedDistribution)
def _(d, data):
    # the data in the base distribution's coordinates; the transforms themselves carry over unchanged
    below = data
    for t in d.transforms[::-1]:
        below = t.inv(below)
    return dist.TransformedDistribution(prefix_condition(d.base_dist, below), list(d.transforms))


@prefix_condition.register(dist.IndependentHMM)
def _(d, data):
    # [..., t, obs] -> one univariate series per base sequence, [..., obs, t, 1]
    per_series = data.transpose(-1, -2).unsqueeze(-1)
    return dist.IndependentHMM(prefix_condition(d.base_dist, per_series))


# ---- reshape_batch ---------------------------------------------------------------------------------------------------
@singledispatch
def reshape_batch(d, batch_shape):
    """``d`` with the batch shape ``batch_shape`` (as many elements as it has now), of the same class."""
    raise _unsupported("reshape_batch()", d)


def _view_under(d, batch_shape):
    batch_shape = tuple(batch_shape)

    def change(v, rank):
        tail = tuple(v.shape[v.dim() - rank:])
        return v.expand(tuple(d.batch_shape) + tail).reshape(batch_shape + tail)
    return _each_tensor(d, change)


for _cls in TENSOR_FAMILIES:
    prefix_condition.register(_cls)(_drop_observed_steps)
    reshape_batch.register(_cls)(_view_under)


@reshape_batch.register(torch.distributions.Independent)
def _(d, batch_shape):
    n = d.reinterpreted_batch_ndims
    return reshape_batch(d.base_dist, tuple(batch_shape) + tuple(d.event_shape[:n])).to_event(n)


@reshape_batch.register(dist.MaskedDistribution)
def _(d, batch_shape):
    keep = d._mask
    if isinstance(keep, torch.Tensor):
        keep = keep.expand(d.batch_shape).reshape(tuple(batch_shape))
    return reshape_batch(d.base_dist, batch_shape).mask(keep)


@reshape_batch.register(torch.distributions.TransformedDistribution)
def _(d, batch_shape):
    base = reshape_batch(d.base_dist, batch_shape)
    before, after = d.base_dist.batch_shape + d.base_dist.event_shape, base.batch_shape + base.event_shape
    return dist.TransformedDistribution(base, [reshape_transform_batch(t, before, after) for t in d.transforms])


@reshape_batch.register(dist.IndependentHMM)
def _(d, batch_shape):
    series = tuple(d.base_dist.batch_shape[-1:])
    return dist.IndependentHMM(reshape_batch(d.base_dist, tuple(batch_shape) + series))


def _only_unit_dims_differ(old, new):
    return [n for n in old if n != 1] == [n for n in new if n != 1]


def _lead_by_view(lead, old, new):
    """The batch dims ``lead`` of one part (right-aligned with the batch shape ``old``) under the move to ``new``,
    which only adds or drops size-1 dims: the part keeps a 1 wherever it was not batched."""
    lead = (1,) * (len(old) - len(lead)) + tuple(lead)
    kept = iter(size for size, n in zip(lead, old) if n != 1)
    return tuple(1 if n == 1 else next(kept) for n in new)


@reshape_batch.register(dist.GaussianHMM)
def _(d, batch_shape):
    old, new = tuple(d.batch_shape), tuple(batch_shape)
    tails = (1, 2, 3, 2, 3, 3, 2, 3)               # event dims of (m0, P0, F, q, Q, H, r, R), the time axis included
    by_view = _only_unit_dims_differ(old, new)
    parts = []
    for i, (p, nd) in enumerate(zip(d._parts, tails)):
        lead, tail = tuple(p.shape[:p.dim() - nd]), tuple(p.shape[p.dim() - nd:])
        if i == 0 and not by_view:                 # the initial mean carries the batch shape for all of them
            p = p.expand(old + tail).reshape(new + tail)
        elif i == 0 or (lead and by_view):
            p = p.reshape(_lead_by_view(lead, old, new) + tail)
        elif any(n != 1 for n in lead):            # another arrangement of the sequences: expand
            p = p.expand(old + tail).reshape(new + tail)
        else:                                      # shared by all sequences: stays one
            p = p.reshape(tail)
        parts.append(p)
    out = dist.GaussianHMM._from_parts(tuple(parts), d.duration, d.__dict__.get("_validate_args"))
    assert out.batch_shape == new and out.event_shape == d.event_shape
    return out


@reshape_batch.register(dist.LinearHMM)
def _(d, batch_shape):
    # the class expands everything eagerly to batch + (time,): its constructor puts the five pieces together again
    # (and peels the observation transforms off a second time), once each is laid out under the new batch shape
    batch_shape = tuple(batch_shape)
    steps = (d.transition_dist.batch_shape[-1],)
    h, o = d.hidden_dim, d.obs_dim
    noise = reshape_batch(d.observation_dist, batch_shape + steps)
    if d.transforms:
        before, after = d.observation_dist.shape(), noise.shape()
        noise = dist.TransformedDistribution(noise, [reshape_transform_batch(t, before, after) for t in d.transforms])
    return dist.LinearHMM(reshape_batch(d.initial_dist, batch_shape),
                          d.transition_matrix.reshape(batch_shape + steps + (h, h)),
                          reshape_batch(d.transition_dist, batch_shape + steps),
                          d.observation_matrix.reshape(batch_shape + steps + (h, o)), noise,
                          validate_args=d.__dict__.get("_validate_args"), duration=d.duration)


# ---- reshape_transform_batch -----------------------------------------------------------------------------------------
@singledispatch
def reshape_transform_batch(t, old_shape, new_shape):
    """The transform ``t`` of a distribution of shape ``old_shape``, for that distribution laid out as ``new_shape``."""
    raise _unsupported("reshape_transform_batch()", t)


def _follow_base(t, old_shape, new_shape):
    moved = {}
    for name in ELEMENTWISE_TRANSFORMS[type(t)]:
        value = getattr(t, name)
        moved[name] = value.expand(old_shape).reshape(new_shape) if isinstance(value, torch.Tensor) else value
    return type(t)(cache_size=t._cache_size, **moved)


for _cls in ELEMENTWISE_TRANSFORMS:
    reshape_transform_batch.register(_cls)(_follow_base)


@reshape_transform_batch.register(dist.transforms.DiscreteCosineTransform)
@reshape_transform_batch.register(dist.transforms.HaarTransform)
def _(t, old_shape, new_shape):
    return t                                       # dim counts from the right, past the batch dims: nothing moves


@reshape_transform_batch.register(transforms.ComposeTransform)
def _(t, old_shape, new_shape):
    return transforms.ComposeTransform([reshape_transform_batch(part, old_shape, new_shape) for part in t.parts])


@reshape_transform_batch.register(transforms._InverseTransform)
def _(t, old_shape, new_shape):
    return reshape_transform_batch(t.inv, old_shape, new_shape).inv
