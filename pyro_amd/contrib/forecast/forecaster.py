"""ForecastingModel and Forecaster (the public interface of the reference's pyro.contrib.forecast.forecaster; the code
is this package's): a model class whose one ``predict(noise_dist, prediction)`` call is an observe statement while
training and a forecast afterwards, and a forecaster that fits it by SVI and then draws sample forecasts.

The noise distribution is where this package's state-space kernels come in: a ``GaussianHMM`` handed to ``predict``
is scored by ONE launch of the Kalman kernel per loss evaluation (util.reshape_batch keeps shared parameters shared),
and a forecast is that class's ``prefix_condition`` (the filter's one launch) followed by its fused draw.

``HMCForecaster`` fits the same models by NUTS, optionally with every time-local latent sampled in a Haar or DCT basis
(``time_reparam``; one launch of pa_time_transform per direction and evaluation).

Not built, and refused by ``Forecaster`` with NotImplementedError when asked for: its ``time_reparam`` option (wrap the
model's ``model`` method in ``poutine.reparam(config=util.time_reparam_dct)`` instead), ``dct_gradients`` and
``subsample_aware`` (DCTAdam), ``warm_start``.  Without a marked parameter the reference's DCTAdam is ClippedAdam,
which is the default optimiser here.
"""
import logging
from abc import ABCMeta, abstractmethod

import torch

from ... import poutine
from ...infer import SVI, Trace_ELBO
from ...infer.autoguide import AutoNormal, init_to_sample
from ...nn import PyroModule
from ...optim import ClippedAdam
from ...poutine.util import site_is_subsample
from ...primitives import plate, sample, subsample
from .util import (PrefixConditionMessenger, PrefixReplayMessenger, reshape_batch, time_reparam_dct,
                   time_reparam_haar)

logger = logging.getLogger(__name__)
RESIDUAL = "residual"                 # the site ``predict`` makes
_UNSUPPORTED = ("time_reparam", "dct_gradients", "subsample_aware", "warm_start")


def _time_steps(d):
    """The number of steps of a distribution over (time, obs): this package's HMM classes keep a time axis of size 1
    in ``event_shape`` for time-homogeneous parameters and name the length by ``duration``."""
    steps = d.event_shape[0]
    while steps == 1 and d is not None:
        if getattr(d, "duration", None) is not None:
            return d.duration
        d = getattr(d, "base_dist", None)
    return steps


def _over_time_and_obs(noise_dist, steps, obs):
    """``noise_dist`` with the event shape (steps, obs): batch dims on the right are expanded where they have to be
    and declared event dims until there are two."""
    missing = 2 - len(noise_dist.event_shape)
    if missing < 0:
        raise ValueError("noise_dist has {} event dims; 0, 1 or 2 can be brought to (time, obs)"
                         .format(len(noise_dist.event_shape)))
    if missing:
        lead = noise_dist.batch_shape[:len(noise_dist.batch_shape) - missing]
        wanted = lead + torch.Size((steps, obs)[:missing])
        if noise_dist.batch_shape != wanted:
            noise_dist = noise_dist.expand(wanted)
        noise_dist = noise_dist.to_event(missing)
    got = (_time_steps(noise_dist), noise_dist.event_shape[-1])
    if got != (steps, obs):
        raise ValueError("noise_dist covers (time, obs) = {}, the prediction {}".format(got, (steps, obs)))
    return noise_dist


class _Run:
    """What one call of a ForecastingModel knows while its ``model`` runs."""

    def __init__(self, data, steps):
        self.data, self.steps = data, steps
        self.time_plate = plate("time", steps, dim=-1)
        self.forecast = None


class _ForecastingModelMeta(type(PyroModule), ABCMeta):
    pass


class ForecastingModel(PyroModule, metaclass=_ForecastingModelMeta):
    """Base class of forecasting models: a subclass writes ``model(zero_data, covariates)``, draws everything that
    depends on time inside ``self.time_plate`` and calls ``self.predict(noise_dist, prediction)`` exactly once,
    outside of it.  Called with data as long as the covariates the model is a training model (the residual is
    observed); called with longer covariates it returns a forecast of the steps in between."""

    def __init__(self):
        super().__init__()
        self._run = None
        self._observed_prefix = {}        # site name -> observed residuals, read by PrefixConditionMessenger

    @abstractmethod
    def model(self, zero_data, covariates):
        """The generative model.  ``zero_data``: zeros of the data's shape, over the duration of the covariates (the
        model may depend on the data's shape and device, not on its values); ``covariates`` [..., duration, features].
        The return value is ignored."""
        raise NotImplementedError

    def _running(self, what):
        if self._run is None:
            raise AssertionError("{} belongs inside .model(): it was used outside of a call of the model".format(what))
        return self._run

    @property
    def time_plate(self):
        """``plate("time", covariates.size(-2), dim=-1)``, inside ``model`` only."""
        return self._running(".time_plate").time_plate

    def predict(self, noise_dist, prediction):
        """The model's observe statement, ``sample("residual", noise_dist, obs=data - prediction)``, for a
        ``noise_dist`` with 0, 1 or 2 event dims that may depend on time (a GaussianHMM or one of its relatives, most
        often) and for data that may end before the prediction does: what lies beyond is then forecast as the
        prediction plus noise drawn from ``noise_dist`` given the residuals seen so far."""
        run = self._running(".predict()")
        if run.forecast is not None:
            raise AssertionError(".predict() may be called once per run of .model()")
        if not isinstance(noise_dist, torch.distributions.Distribution) or not isinstance(prediction, torch.Tensor):
            raise TypeError("predict(noise_dist, prediction) takes a distribution and a tensor")
        steps, obs = prediction.shape[-2:]
        noise_dist = _over_time_and_obs(noise_dist, steps, obs)
        # time is an event dim now.  Where it was a batch dim, everything else in the trace still has the time plate's
        # dim: a batch dim of size 1 goes there, on the distribution, the data and the prediction alike
        noise_dist = reshape_batch(noise_dist, tuple(noise_dist.batch_shape) + (1,))
        data = subsample(run.data.unsqueeze(-3), event_dim=2)
        prediction = prediction.unsqueeze(-3)
        seen = data.size(-2)
        if seen == steps:
            sample(RESIDUAL, noise_dist, obs=data - prediction)
            ahead = data.new_zeros(data.shape[:-2] + (0, obs))
        else:
            # PrefixConditionMessenger, installed by the Forecaster around the model, finds the residuals here while
            # the site is sampled and swaps the distribution for the conditional one
            self._observed_prefix[RESIDUAL] = data - prediction.narrow(-2, 0, seen)
            try:
                noise = sample(RESIDUAL, noise_dist)
            finally:
                self._observed_prefix.pop(RESIDUAL, None)
            future = prediction.narrow(-2, seen, steps - seen)
            if noise.shape[-data.dim():] != future.shape[-data.dim():]:
                raise ValueError("the residual site returned {} for a forecast of {}: is PrefixConditionMessenger "
                                 "installed?".format(tuple(noise.shape), tuple(future.shape)))
            ahead = future + noise
        run.forecast = ahead.squeeze(-3)

    def forward(self, data, covariates):
        if data.dim() < 2 or covariates.dim() < 2 or data.size(-2) > covariates.size(-2):
            raise ValueError("expected data [..., t, obs] and covariates [..., duration >= t, features], got {} and {}"
                             .format(tuple(data.shape), tuple(covariates.shape)))
        steps = covariates.size(-2)
        self._run = run = _Run(data, steps)
        try:
            self.model(data.new_zeros(()).expand(data.shape[:-2] + (steps, data.size(-1))), covariates)
        finally:
            self._run = None
        if run.forecast is None:
            raise AssertionError(".model() has to call .predict()")
        return run.forecast


class Forecaster(torch.nn.Module):
    """Fits ``model`` to ``(data, covariates)`` by SVI -- variational inference over the latent variables, exact
    inference over the noise distribution -- and then, called with data and LONGER covariates, draws sample forecasts
    of the steps in between.

    ``losses``: the loss of every training step per data element, ``-elbo / data.numel()``.

    Arguments as the reference's: ``guide`` (default ``AutoNormal(model, init_loc_fn=init_loc_fn,
    init_scale=init_scale, create_plates=create_plates)``), ``optim`` (default ClippedAdam with ``learning_rate``,
    ``betas``, ``clip_norm`` and a per-step decay of ``learning_rate_decay ** (1 / num_steps)``), ``num_steps``,
    ``num_particles``, ``vectorize_particles``, ``log_every``.

    Training steps are eager ones (``SVI(..., hip_graph=False)``): a forecasting model subsamples through
    ``create_plates`` and may draw on the host, which a step captured into a hipGraph would freeze."""

    def __init__(self, model, data, covariates, *, guide=None, init_loc_fn=init_to_sample, init_scale=0.1,
                 create_plates=None, optim=None, learning_rate=0.01, betas=(0.9, 0.99), learning_rate_decay=0.1,
                 clip_norm=10.0, time_reparam=None, dct_gradients=False, subsample_aware=False, num_steps=1001,
                 num_particles=1, vectorize_particles=True, warm_start=False, log_every=100):
        super().__init__()
        asked = dict(time_reparam=time_reparam, dct_gradients=dct_gradients, subsample_aware=subsample_aware,
                     warm_start=warm_start)
        for option in _UNSUPPORTED:
            if asked[option]:
                raise NotImplementedError("Forecaster({}={!r}) is not supported".format(option, asked[option]))
        if data.size(-2) != covariates.size(-2):
            raise ValueError("training needs covariates as long as the data: {} steps against {}"
                             .format(covariates.size(-2), data.size(-2)))
        self.model = model
        self.guide = guide if guide is not None else AutoNormal(
            model, init_loc_fn=init_loc_fn, init_scale=init_scale, create_plates=create_plates)

        elbo = Trace_ELBO(num_particles=num_particles, vectorize_particles=vectorize_particles)
        elbo._guess_max_plate_nesting(model, self.guide, (data, covariates), {})
        # dim -1 is the time plate's, also for a model that draws nothing inside it: vectorised particles go left of it
        elbo.max_plate_nesting = max(elbo.max_plate_nesting, 1 + elbo._particle_dims)
        self.max_plate_nesting = elbo.max_plate_nesting
        self.losses = []
        if num_steps:
            if optim is None:
                optim = ClippedAdam({"lr": learning_rate, "betas": betas, "clip_norm": clip_norm,
                                     "lrd": learning_rate_decay ** (1 / num_steps)})
            svi = SVI(model, self.guide, optim, elbo, hip_graph=False)
            for step in range(num_steps):
                self.losses.append(svi.step(data, covariates) / data.numel())
                if log_every and step % log_every == 0:
                    logger.info("step %4d loss = %0.6g", step, self.losses[-1])
        if hasattr(self.guide, "create_plates"):
            self.guide.create_plates = None          # forecasts are for every series

    def __call__(self, data, covariates, num_samples, batch_size=None):
        """Sample forecasts of the steps ``[t1, t2)``, ``t1 = data.size(-2)`` and ``t2 = covariates.size(-2)``: a
        tensor of shape ``(num_samples, 1, ..., 1) + data.shape[:-2] + (t2 - t1, data.size(-1))``, the 1's keeping
        the sample dim clear of the model's plates.  ``batch_size``: draw that many at a time."""
        return super().__call__(data, covariates, num_samples, batch_size)

    def forward(self, data, covariates, num_samples, batch_size=None):
        if not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError("num_samples must be a positive int, got {!r}".format(num_samples))
        if data.size(-2) > covariates.size(-2):
            raise ValueError("the covariates end before the data do")
        if batch_size is not None:
            sizes = [batch_size] * (num_samples // batch_size) + [num_samples % batch_size]
            return torch.cat([self._draw(data, covariates, n) for n in sizes if n])
        return self._draw(data, covariates, num_samples)

    @torch.no_grad()
    def _draw(self, data, covariates, n):
        """``n`` forecasts: the guide's draw of the latents over the observed steps, then the model replayed on it."""
        if self.max_plate_nesting < 1:
            raise ValueError("max_plate_nesting must leave room for the time plate")
        particles = dict(name="particles", size=n, dim=-1 - self.max_plate_nesting)
        with poutine.block(), poutine.trace() as latents, plate(**particles):
            self.guide(data, covariates)
        if data.size(-2) == covariates.size(-2):
            handlers = [poutine.replay(trace=latents.trace)]
        else:
            handlers = [PrefixReplayMessenger(latents.trace), PrefixConditionMessenger(self.model._observed_prefix)]
        def run():
            with plate(**particles):
                return self.model(data, covariates)

        for handler in reversed(handlers):
            run = handler(run)
        return run()


_TIME_REPARAMS = {"dct": time_reparam_dct, "haar": time_reparam_haar}
_REPLAY_BATCH = 256          # posterior draws pushed back through the reparameterised model at a time


def _latent_sites(trace):
    return [name for name, site in trace.nodes.items()
            if site["type"] == "sample" and not site["is_observed"] and not site_is_subsample(site)]


class HMCForecaster(torch.nn.Module):
    """Fits ``model`` to ``(data, covariates)`` by this package's ``MCMC(NUTS(model))`` and then, called with data and
    LONGER covariates, draws sample forecasts with ``Forecaster``'s contract and output shape.

    ``time_reparam``: None, ``"dct"`` or ``"haar"``: every unobserved site inside the time plate is sampled as its
    DCT or Haar coefficients along time (``util.time_reparam_dct`` / ``util.time_reparam_haar``), which takes a random
    walk's correlations out of the geometry NUTS sees.  On the device each evaluation of the model then runs one
    launch of pa_time_transform per such site and one more for its gradient.  Anything else raises ValueError.
    ``num_warmup``, ``num_samples``, ``num_chains``, ``dense_mass`` (NUTS ``full_mass``) and ``max_tree_depth`` as
    the reference's.

    ``jit_compile`` is passed to ``NUTS``, where it captures the sampler's rounds in hipGraphs.  Known open fault: a
    captured step that contains the GaussianHMM launch has ended in a segmentation fault inside the runtime
    ("contrib.forecast"); leave it off for a model whose noise is one of the HMM classes.

    Deviation from the reference, on purpose.  The reference replays the REPARAMETERISED model at forecast time, so
    that PrefixReplayMessenger splices the ``t1`` posterior coefficients onto ``t2 - t1`` prior coefficients in the
    frequency (or wavelet) domain, which stretches the fitted latent over the longer window.  Here the posterior draws
    of the ORIGINAL sites are computed once, after the run: the reparameterised model is replayed on the chain's draws
    in batches and its Delta sites are read.  ``samples`` keeps those time-domain draws ({site: [draws, ...]}, laid out
    under the particle plate), and a forecast replays the user's own model on them: the time-domain prefix, then the
    prior for the steps ahead."""

    def __init__(self, model, data, covariates=None, *, num_warmup=1000, num_samples=1000, num_chains=1,
                 time_reparam=None, dense_mass=False, jit_compile=False, max_tree_depth=10):
        super().__init__()
        from ...infer.mcmc import MCMC, NUTS
        from ...infer.mcmc.util import _guess_max_plate_nesting
        if time_reparam is not None and time_reparam not in _TIME_REPARAMS:
            raise ValueError("unknown time_reparam: {!r} (None, 'dct' or 'haar')".format(time_reparam))
        if covariates is None:
            covariates = data.new_empty(data.shape[:-1] + (0,))
        if data.size(-2) != covariates.size(-2):
            raise ValueError("training needs covariates as long as the data: {} steps against {}"
                             .format(covariates.size(-2), data.size(-2)))
        self.model = model
        sampled = model if time_reparam is None else poutine.reparam(model, config=_TIME_REPARAMS[time_reparam])
        args = (data, covariates)
        # dim -1 is the time plate's, also for a model that draws nothing inside it
        self.max_plate_nesting = max(_guess_max_plate_nesting(model, args, {}),
                                     _guess_max_plate_nesting(sampled, args, {}), 1)
        kernel = NUTS(sampled, full_mass=dense_mass, jit_compile=jit_compile, ignore_jit_warnings=True,
                      max_tree_depth=max_tree_depth, max_plate_nesting=self.max_plate_nesting)
        mcmc = MCMC(kernel, num_samples=num_samples, warmup_steps=num_warmup, num_chains=num_chains)
        mcmc.run(*args)
        self.diagnostics = mcmc.diagnostics
        self.samples = self._time_domain(sampled, args, mcmc.get_samples())
        self._num_draws = num_samples * num_chains
        # the trace forecasts are replayed from: the user's model under a particle plate of size 1, latent sites only
        with poutine.block(), poutine.trace() as seen, self._particles(1):
            model(*args)
        self._trace = seen.trace
        for name in list(self._trace.nodes):
            if name not in self.samples:
                self._trace.remove_node(name)

    def _particles(self, n):
        return plate("particles", n, dim=-1 - self.max_plate_nesting)

    @torch.no_grad()
    def _time_domain(self, sampled, args, draws):
        """The chain's draws of the sites NUTS moved -> draws of the user's model's own latent sites, [draws, ...]
        under the particle plate: the sampled model is run on the draws, _REPLAY_BATCH at a time, and the values of
        the original sites (Delta sites where they were reparameterised) are read."""
        with poutine.block():
            wanted = _latent_sites(poutine.trace(self.model).get_trace(*args))
            proto = poutine.trace(sampled).get_trace(*args)
        batch_ndims = {name: len(proto.nodes[name]["fn"].batch_shape) for name in draws}
        total = next(iter(draws.values())).size(0) if draws else 0
        pieces = {name: [] for name in wanted}
        for start in range(0, total, _REPLAY_BATCH):
            fixed = {}
            for name, v in draws.items():
                v = v[start:start + _REPLAY_BATCH]
                pad = self.max_plate_nesting - batch_ndims[name]
                fixed[name] = v.reshape(v.shape[:1] + (1,) * pad + v.shape[1:])
            n = next(iter(fixed.values())).size(0)

            def run():
                with self._particles(n):
                    return sampled(*args)
            with poutine.block():
                tr = poutine.trace(poutine.condition(run, data=fixed)).get_trace()
            for name in wanted:
                value = tr.nodes[name]["value"]
                pieces[name].append(value.expand((n,) + tuple(value.shape[1:])) if value.size(0) != n else value)
        return {name: torch.cat(vs) for name, vs in pieces.items() if vs}

    def __call__(self, data, covariates, num_samples, batch_size=None):
        """Sample forecasts of the steps ``[t1, t2)``, ``t1 = data.size(-2)`` and ``t2 = covariates.size(-2)``: a
        tensor of shape ``(num_samples, 1, ..., 1) + data.shape[:-2] + (t2 - t1, data.size(-1))``.  ``batch_size``:
        draw that many at a time."""
        return super().__call__(data, covariates, num_samples, batch_size)

    def forward(self, data, covariates, num_samples, batch_size=None):
        if not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError("num_samples must be a positive int, got {!r}".format(num_samples))
        if data.size(-2) > covariates.size(-2):
            raise ValueError("the covariates end before the data do")
        if batch_size is not None:
            sizes = [batch_size] * (num_samples // batch_size) + [num_samples % batch_size]
            return torch.cat([self._draw(data, covariates, n) for n in sizes if n])
        return self._draw(data, covariates, num_samples)

    @torch.no_grad()
    def _draw(self, data, covariates, n):
        """``n`` forecasts: posterior draws of the latents over the observed steps, picked at random (without
        replacement while there are enough), then the user's model replayed on them."""
        weights = torch.ones(self._num_draws, device=data.device)
        picked = torch.multinomial(weights, n, replacement=n > self._num_draws)
        for name, node in self._trace.nodes.items():
            node["value"] = self.samples[name].index_select(0, picked)
        if data.size(-2) == covariates.size(-2):
            handlers = [poutine.replay(trace=self._trace)]
        else:
            handlers = [PrefixReplayMessenger(self._trace), PrefixConditionMessenger(self.model._observed_prefix)]

        def run():
            with self._particles(n):
                return self.model(data, covariates)

        for handler in reversed(handlers):
            run = handler(run)
        return run()
