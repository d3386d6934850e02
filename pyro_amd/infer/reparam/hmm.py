"""Auxiliary-variable reparameteriser of LinearHMM sites (role of pyro/infer/reparam/hmm.py): the component
reparameterisers give the initial, transition and observation noise auxiliary variables conditioned on which each is
Gaussian, and the site becomes a ``GaussianHMM`` -- whose ``log_prob``, with its gradients, is one launch of the Kalman
filter kernel.  Per-step noise scales arrive there as per-step diagonal covariances, which that kernel takes as they
are."""
from ... import distributions as dist
from .reparam import Reparam


class LinearHMMReparam(Reparam):
    """``init``, ``trans``, ``obs``: optional reparameterisers (e.g. ``StudentTReparam``) for the three noise
    distributions of a ``LinearHMM`` (or of the ``LinearHMM`` inside an ``IndependentHMM``); a component left out
    must be Gaussian already.  Their auxiliary sites are named ``<name>_init``, ``<name>_trans`` and ``<name>_obs``
    (plus whatever the component appends).  Transition and observation distributions are expanded to the duration
    first, so every step gets its own auxiliary variable; the observation's reparameteriser sees the site's value.
    Observation transforms of the ``LinearHMM`` wrap the resulting ``GaussianHMM`` in a ``TransformedDistribution``."""

    def __init__(self, init=None, trans=None, obs=None):
        assert init is None or isinstance(init, Reparam)
        assert trans is None or isinstance(trans, Reparam)
        assert obs is None or isinstance(obs, Reparam)
        self.init, self.trans, self.obs = init, trans, obs

    def apply(self, msg):
        name, value, is_observed = msg["name"], msg["value"], msg["is_observed"]
        fn, event_dim = self._unwrap(msg["fn"])
        assert isinstance(fn, (dist.LinearHMM, dist.IndependentHMM)), type(fn).__name__
        if fn.duration is None:
            raise ValueError("LinearHMMReparam requires duration to be specified on targeted LinearHMM distributions")

        if isinstance(fn, dist.IndependentHMM):
            indep_value = None if value is None else value.transpose(-1, -2).unsqueeze(-1)
            new = self.apply({"name": name, "fn": dist.Independent(fn.base_dist, 1), "value": indep_value,
                              "is_observed": is_observed})
            hmm = dist.IndependentHMM(new["fn"].to_event(-1))
            if new["value"] is not indep_value:
                value = new["value"].squeeze(-1).transpose(-1, -2)
            return {"fn": hmm, "value": value, "is_observed": is_observed}

        init_dist = fn.initial_dist
        if self.init is not None:
            new = self.init.apply({"name": name + "_init", "fn": self._wrap(init_dist, event_dim - 1), "value": None,
                                   "is_observed": False})
            init_dist = new["fn"].to_event(1 - new["fn"].event_dim)

        trans_dist = fn.transition_dist
        if self.trans is not None:
            if trans_dist.batch_shape[-1] != fn.duration:
                trans_dist = trans_dist.expand(trans_dist.batch_shape[:-1] + (fn.duration,))
            new = self.trans.apply({"name": name + "_trans", "fn": self._wrap(trans_dist, event_dim), "value": None,
                                    "is_observed": False})
            trans_dist = new["fn"].to_event(1 - new["fn"].event_dim)

        obs_dist = fn.observation_dist
        if self.obs is not None:
            if obs_dist.batch_shape[-1] != fn.duration:
                obs_dist = obs_dist.expand(obs_dist.batch_shape[:-1] + (fn.duration,))
            new = self.obs.apply({"name": name + "_obs", "fn": self._wrap(obs_dist, event_dim), "value": value,
                                  "is_observed": is_observed})
            obs_dist = new["fn"].to_event(1 - new["fn"].event_dim)
            value, is_observed = new["value"], new["is_observed"]

        hmm = dist.GaussianHMM(init_dist, fn.transition_matrix, trans_dist, fn.observation_matrix, obs_dist,
                               duration=fn.duration)
        hmm = self._wrap(hmm, event_dim)
        if fn.transforms:
            hmm = dist.TransformedDistribution(hmm, fn.transforms)
        return {"fn": hmm, "value": value, "is_observed": is_observed}
