"""infer_discrete: run a model with its enumerated discrete sites set to one joint draw from their posterior
(temperature 1) or to a most probable joint assignment (temperature 0) given everything else in the trace
(reference: pyro/infer/discrete.py:41-170 _sample_posterior / _sample_posterior_from_trace / infer_discrete, which
run the sum-product once more with the sample / map einsum backends of pyro/ops/einsum/ and read the values back).

Two routes, site by site in the order the model visits them:
  * generic -- any model TraceEnum_ELBO can enumerate: the site's conditional given the sites already fixed is the
    gradient of the log-partition function with respect to a probe on the site's log-factor (the machinery of
    TraceEnum_ELBO.sample_posterior, infer/traceenum_elbo.py).  At temperature 1 that is the posterior, and the value
    is its inverse CDF at one Philox uniform per element; at temperature 0 the contraction runs as max-product
    (ops/contract.py::max_product) and the gradient is the indicator of a most probable value that the sites fixed so
    far can be extended with -- fixing the sites one after another therefore ends at a joint maximiser, ties included;
  * fast -- a plated mixture: the site's factors are exactly its own prior (constant along the data plate or per row)
    and ONE observed family term the mixture leaf matches (scalar data of kernels.MIXTURE_FAMILIES, or a diagonal
    Normal over at most 8 features; with weights shared by the rows also any of those families over at most 1024
    features through ``.to_event(1)`` and a full-covariance MultivariateNormal over at most 64; an outer plate of
    parameter sets is optional): kernels.mixture_assign* picks or draws every row's component in one pass, and
    nothing of size K N (let alone K N D) exists beyond the caller's own per-row weights.
    ``ops.contract.FUSED_MIXTURE = False`` turns it off;
  * fast -- a ``pyro.markov`` chain: the sites of one component of the enumerated factor graph form a simple path in
    the order the model declares them, none of them fixed yet, all in one plate context (factors under deeper plates --
    observations in a plate nested inside -- are product-reduced to it first), at most 64 states, float32 / float64 on
    the device.  When the chain's first site is asked for, kernels.logchain_decode fixes all T of them in ONE launch
    -- backward max / log-sum-exp messages, then every state given the one before: the Viterbi path at temperature 0,
    a joint posterior draw at temperature 1 -- in O(T K^2) per sequence with a [B, T, K] workspace, where the generic
    route contracts the whole chain once per site; the later sites read the kept values.  The T steps' uniforms are
    reserved in one go as T reservations of one uniform per sequence would be.  Anything else -- a tree, a site shared
    by two chains, more than 64 states, a chain with a state already fixed or conditioned -- stays on the generic
    route.  ``ops.contract.FUSED_CHAIN = False`` turns it off.
Both routes draw from the same uniforms in the same way, so at a fixed seed they return the same values -- for a chain
as long as no other drawing site is visited between the chain's sites: the generic route reserves a site's uniforms
when it visits the site, the chain route all T sites' at the first; with sites interleaved the result is still one
joint posterior draw, from other uniforms.
"""
import functools
import warnings

import torch

from .. import kernels, poutine, rng
from ..ops import contract
from ..poutine.util import prune_subsample_sites
from .traceenum_elbo import (BackwardSample, _enum_factors, _enum_log_prob, _enum_sites, _evidence_of, _lazy_family,
                             _ordinal, _packed, _posterior_of, _posterior_weights, _support_last)


def _wide_assign_ready(x):
    """Whether the wide leaves' assignment kernels (kernels.mixture_assign_event / mixture_assign_mvn) can take the
    observation ``x``: they run on the device only."""
    return x.is_cuda


def _chain_decode_ready(t):
    """Whether the chain decoding kernel (kernels.logchain_decode) can take the potentials ``t``: it runs on the
    device only."""
    return t.is_cuda


def _uniform(shape, dtype, device, on_device):
    """One uniform per element of ``shape`` in row-major order: the Philox stream on the device, torch's generator
    elsewhere."""
    if on_device:
        return rng.uniform(tuple(shape), dtype, device)
    return torch.rand(tuple(shape), dtype=dtype, device=device)


def inverse_cdf(probs, u):
    """The smallest k with c_k > u c_{K-1}, c = cumsum(probs) along the last dim, clamped to the largest k with
    probs_k > 0; 0 where the row has no positive (or a NaN) entry.  probs [.., K] >= 0, u [..] -> int64 [..]."""
    K = probs.shape[-1]
    p = torch.nan_to_num(probs, nan=0.0)
    c = torch.cumsum(p, -1)
    ks = torch.arange(K, device=p.device)
    first = torch.where(c > u.unsqueeze(-1) * c[..., -1:], ks, ks.new_full((), K)).min(-1).values
    last = torch.where(p > 0, ks, ks.new_full((), -1)).max(-1).values
    z = torch.minimum(first, last).clamp(min=0)
    return torch.where(torch.isnan(probs).any(-1), torch.zeros_like(z), z)


def _value_of(fn, index, support):
    """The site's value for the support indices ``index``: the index itself (Categorical), 0. / 1. (Bernoulli) or the
    one-hot vector (OneHotCategorical)."""
    import torch.distributions as td
    base = fn
    while hasattr(base, "base_dist"):
        base = base.base_dist
    if isinstance(base, td.Bernoulli):
        return index.to(support.dtype)
    if isinstance(base, td.OneHotCategorical):
        return torch.nn.functional.one_hot(index, support.shape[-1]).to(support.dtype)
    if isinstance(base, td.Categorical):
        return index
    raise NotImplementedError("infer_discrete of an enumerated {} site".format(type(base).__name__))


def _enum_ids_of(site, first_enum_dim):
    """The ids of the enumerated variables that the site's log-probability depends on, read off the shapes of its
    distribution and value (nothing is evaluated)."""
    fn, v = site["fn"], site["value"]
    ev = len(getattr(fn, "event_shape", ()))
    shapes = [tuple(getattr(fn, "batch_shape", ()))]
    if isinstance(v, torch.Tensor):
        shapes.append(tuple(v.shape[:v.dim() - ev]))
    dim_to_id = site["infer"].get("_dim_to_id", {})
    ids = set()
    for shp in shapes:
        n = len(shp)
        for i, s_ in enumerate(shp):
            if s_ > 1 and i - n <= first_enum_dim:
                ids.add(dim_to_id.get(i - n, ("?", site["name"], i - n)))      # (unknown dim: matches no site)
    return ids


class _InferDiscrete(BackwardSample):
    """BackwardSample that sets the value of every enumerated site itself: argmax of the max-marginal (temperature 0)
    or the inverse CDF of the posterior at Philox uniforms (temperature 1), by the mixture_assign kernels where the
    site is the assignment of a plated mixture."""

    def __init__(self, model_trace, enum_names, enum_ids, temperature):
        super().__init__(model_trace, enum_names, enum_ids)
        self.temperature = temperature
        self._fixed = {}                  # values set so far whose evidence tensors nobody has asked for yet
        self._decoded = {}                # support indices of a chain's sites, kept from its one launch

    def _choose(self, msg):
        name = msg["name"]
        site = self.model_trace.nodes[name]
        index = self._decoded.pop(name, None)
        if index is None:
            index = self._fast(name, site)
        if index is None:
            index = self._decode(name, site)
        if index is None:
            index = self._generic(name)
        msg["value"] = _value_of(site["fn"], index, site["value"])

    def _pyro_post_sample(self, msg):
        # (the indicator of a value is a tensor of the site's enumerated shape, [K, N] for a mixture's assignment: it
        #  is built only when a later site takes the generic route)
        if msg["name"] in self.enum_names and not msg["is_observed"]:
            self._fixed[msg["name"]] = msg["value"]

    def _generic(self, name):
        while self._fixed:
            fixed, value = self._fixed.popitem()
            self.evidence[fixed] = _evidence_of(self.model_trace.nodes[fixed], value)
        args = (self.model_trace, self.enum_names, self.enum_ids, name, self.evidence)
        if self.temperature == 0:
            with contract.max_product():
                g = _posterior_weights(*args)
            return torch.argmax(_support_last(self.model_trace, name, g), -1)
        probs = _posterior_of(*args).detach()
        u = _uniform(probs.shape[:-1], probs.dtype, probs.device, kernels.on_device(probs))
        return inverse_cdf(probs, u)

    def _decode(self, name, site):
        """The site's support indices from kernels.logchain_decode when the site is the first of a pyro.markov chain
        the kernel takes (the other sites' indices are kept for their turn), else None."""
        if not contract.FUSED_CHAIN or name in self.evidence or name in self._fixed:
            return None
        trace = self.model_trace
        name_of = {trace.nodes[n]["infer"]["_dim_to_id"][trace.nodes[n]["infer"]["_enumerate_dim"]]: n
                   for n in self.enum_names}
        kid = site["infer"]["_dim_to_id"][site["infer"]["_enumerate_dim"]]
        factors = _enum_factors(trace, self.enum_names, self.enum_ids, {})
        every = [t for terms in factors.values() for t in terms]
        found = [(terms, ids) for terms, ids in contract._partition(every, set(self.enum_ids)) if kid in ids]
        if len(found) != 1:
            return None
        terms, ids = found[0]
        ordinal = _ordinal(site)
        if len(ids) < 3 or any(v not in name_of or name_of[v] in self.evidence or name_of[v] in self._fixed
                               or _ordinal(trace.nodes[name_of[v]]) != ordinal for v in ids):
            return None                       # (a state already fixed, or sites in different plate contexts)
        reduced = []
        for t in terms:
            if not set(t.ids) <= ids or not t.ordinal >= ordinal:
                return None
            # factors below the chain's plates (observations in a plate nested inside): their plate product first
            tensor = contract._product(t.dense(), t.ordinal - ordinal) if t.ordinal != ordinal else t.dense()
            reduced.append(contract.Term(tensor.detach(), t.ids, ordinal))
        match = contract._match_chain(reduced, ids, ready=_chain_decode_ready)
        if match is None:
            return None
        order, U, P, batch = match
        declared = [n for n in trace.nodes if n in self.enum_names and n in {name_of[v] for v in ids}]
        along = [name_of[v] for v in order]
        if along == declared[::-1]:           # the path was walked from its other end
            U, P = U.flip(1).contiguous(), P.flip(1).transpose(-1, -2).contiguous()
        elif along != declared:
            return None
        if declared[0] != name:
            return None
        B, T, _ = U.shape
        if self.temperature == 1:
            per = 4 if U.dtype == torch.float32 else 2    # uniforms per Philox block: rng.reserve's rule
            blocks = (B + per - 1) // per
            seed, off, off_dev = rng.reserve_blocks(T * blocks)
        else:
            blocks, seed, off, off_dev = 0, 0, 0, None
        z, _ = kernels.logchain_decode(U, P, mode=self.temperature, seed=seed, offset=off, offset_dev=off_dev,
                                       step_blocks=blocks)
        shape = tuple(batch)
        while shape and shape[0] == 1:        # (as _support_last shapes the generic route's indices)
            shape = shape[1:]
        for t, n in enumerate(declared):
            self._decoded[n] = z[:, t].reshape(shape)
        return self._decoded.pop(name)

    def _fast(self, name, site):
        """The site's support indices from kernels.mixture_assign*, shaped like the site's plates, or None when the
        site is not the assignment of a plated mixture the kernels take."""
        if not contract.FUSED_MIXTURE or name in self.evidence or name in self._fixed:
            return None
        trace = self.model_trace
        fed = trace._first_enum_dim
        kid = site["infer"]["_dim_to_id"][site["infer"]["_enumerate_dim"]]
        if _enum_ids_of(site, fed) != {kid}:
            return None                       # (a discrete parent in the prior: the factor is shared)
        lazy = None
        for other, node in trace.nodes.items():
            if node["type"] != "sample" or other == name or kid not in _enum_ids_of(node, fed):
                continue
            if lazy is not None or other in self.enum_names:
                return None                   # a second factor, or a second enumerated site sharing one
            got = _lazy_family(node, fed)
            if got is None or got[0] != kid:
                return None
            lazy = contract.Term(None, (kid,), _ordinal(node), lazy=got[1])
        if lazy is None or lazy.ordinal != _ordinal(site):
            return None
        lz = lazy.lazy
        mvn = isinstance(lz, contract.LazyMvn)
        diag = not mvn and lz.D is not None and lz.dist_id == kernels._lib.DIST_NORMAL and lz.D <= kernels.MIXTURE_MAX_D
        wide = lz.D is not None and not diag  # an event-shaped or full-covariance leaf: weights shared by the rows
        if wide and not (_wide_assign_ready(lz.value) and
                         lz.D <= (kernels.MIXTURE_MVN_MAX_D if mvn else kernels.MIXTURE_EVENT_MAX_D)):
            return None
        own = _packed(site, _enum_log_prob(site).detach(), fed)
        match = contract._match_mixture([own, lazy], {kid}, lazy.ordinal)
        if match is None:
            return None
        _, a, a_rows, _ = match
        if wide and (a_rows is not None or a is None):
            return None
        x, K, B = lz.value, lz.K, lz.B
        N = x.shape[0]
        if a_rows is not None:
            w = (a_rows if a is None else a_rows + a.unsqueeze(1)).expand(B, N, K)
        else:
            w = a.expand(B, K)
        seed, off, off_dev = rng.reserve(B * N, x.dtype) if self.temperature == 1 else (0, 0, None)
        if mvn:
            # W = L^-1 formed in float64, as the contraction forms it for the leaf (contract._try_fused_mixture)
            L = lz.scale_tril.detach().transpose(0, 1)
            eye = torch.eye(lz.D, dtype=torch.float64, device=L.device)
            W = torch.linalg.solve_triangular(L.to(torch.float64), eye, upper=False).to(x.dtype)
            z = kernels.mixture_assign_mvn(x.contiguous(), w.contiguous(),
                                           lz.loc.detach().transpose(0, 1).contiguous(), W.contiguous(),
                                           mode=self.temperature, seed=seed, offset=off, offset_dev=off_dev)
        elif wide:
            p1 = None if lz.p1 is None else lz.p1.detach().transpose(0, 1).contiguous()
            z = kernels.mixture_assign_event(int(lz.dist_id), x.contiguous(), w.contiguous(),
                                             lz.p0.detach().transpose(0, 1).contiguous(), p1,
                                             mode=self.temperature, seed=seed, offset=off, offset_dev=off_dev)
        elif diag:
            z = kernels.mixture_assign_diag_normal(x.contiguous(), w, lz.p0.detach().transpose(0, 1).contiguous(),
                                                   lz.p1.detach().transpose(0, 1).contiguous(),
                                                   mode=self.temperature, seed=seed, offset=off, offset_dev=off_dev)
        else:
            p0, s0, bs0 = contract._flat_param(None if lz.p0 is None else lz.p0.detach(), K, B)
            p1, s1, bs1 = contract._flat_param(None if lz.p1 is None else lz.p1.detach(), K, B)
            if p0 is False or p1 is False or p0 is None:
                return None
            z = kernels.mixture_assign(int(lz.dist_id), x.contiguous(), w, p0, s0, p1, s1, bs0, bs1,
                                       mode=self.temperature, seed=seed, offset=off, offset_dev=off_dev)
        if lz.batch_dim is None:
            return z.reshape(N)
        return z.reshape((B,) + (1,) * (-lz.batch_dim - 2) + (N,))


def _sample_posterior(model, first_available_dim, temperature, strict_enumeration_warning, *args, **kwargs):
    with poutine.block():
        enum_trace = poutine.trace(poutine.enum(model, first_available_dim=first_available_dim)).get_trace(
            *args, **kwargs)
    enum_trace = prune_subsample_sites(enum_trace)
    enum_trace._first_enum_dim = first_available_dim
    enum_names, enum_ids = _enum_sites(enum_trace, poutine.Trace())
    enum_names = [n for n in enum_names if not enum_trace.nodes[n]["is_observed"]]
    if not enum_names:
        if strict_enumeration_warning:
            warnings.warn("infer_discrete found no sample sites configured for enumeration. If you want to enumerate "
                          "sites, you need to @config_enumerate or set infer={\"enumerate\": \"parallel\"}.")
        return model(*args, **kwargs)
    with torch.no_grad(), _InferDiscrete(enum_trace, enum_names, enum_ids, temperature):
        return model(*args, **kwargs)


def infer_discrete(fn=None, first_available_dim=None, temperature=1, *, strict_enumeration_warning=True):
    """A version of ``fn`` whose model-side enumerated sites (``infer={"enumerate": "parallel"}``,
    ``config_enumerate``) are set to one joint draw from their posterior given everything else in the trace
    (``temperature=1``) or to a joint maximiser of that posterior (``temperature=0``: MAP, for a ``pyro.markov`` chain
    the Viterbi path); it returns what ``fn`` returns.  Usable as a wrapper and as a decorator with arguments.
    Continuous sites are fixed from outside: ``infer_discrete(poutine.replay(model, trace=guide_trace), ...)`` or
    ``poutine.condition``.  ``first_available_dim``: the first tensor dim (negative, left of every plate dim) that
    enumeration may use (reference: pyro/infer/discrete.py:120-170)."""
    if temperature not in (0, 1):
        raise ValueError("infer_discrete: temperature must be 0 (most probable) or 1 (a draw), got {!r}"
                         .format(temperature))
    if first_available_dim is None or first_available_dim >= 0:
        raise ValueError("infer_discrete: first_available_dim must be negative, got {!r}".format(first_available_dim))
    if fn is None:                                     # used as a decorator with arguments
        return functools.partial(infer_discrete, first_available_dim=first_available_dim, temperature=temperature,
                                 strict_enumeration_warning=strict_enumeration_warning)
    return functools.partial(_sample_posterior, fn, first_available_dim, temperature, strict_enumeration_warning)

