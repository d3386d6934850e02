"""Hidden Markov models with time included in the event shape.

DiscreteHMM: discrete latent state and arbitrary observation distribution (reference:
pyro/distributions/hmm.py:243-420).

The reference eliminates the time axis with a parallel-scan of log-space matrix products
(_sequential_logmatmulexp, O(log T) steps of [K, K] x [K, K] products and their autograd duals).
Here log_prob is ONE launch of the forward-backward kernel (pa_logchain_fwd_bwd): the initial state
is variable 0 of a chain of T + 1 variables, step t contributes the transition as the pairwise
potential and the observation log-likelihood as the unary potential of variable t + 1; the launch
returns the log-likelihood of every batch element and, as its gradient, the posterior marginals.

GaussianHMM: linear-Gaussian state-space model (reference: pyro/distributions/hmm.py:434-741).  The reference
eliminates time with sequential_gaussian_tensordot (O(log T) rounds of batched Gaussian contractions); here
log_prob is ONE launch of the Kalman filter kernel (pa_gaussian_hmm_fwd_bwd), whose backward pass -- the adjoint
of the filter's own steps -- hands back the gradient with respect to every parameter and the data;
rsample_posterior is the same filter followed by a backward-sampling sweep (pa_gaussian_hmm_sample); smooth is the
same filter followed by the Rauch-Tung-Striebel sweep, the smoothed marginals of every state in ONE launch
(pa_gaussian_hmm_smooth); rsample factors every distinct covariance once
and runs one lane per sample path (pa_gaussian_hmm_draw).  Whatever the kernels do
not take -- CPU tensors, hidden or obs dimension over 16, other dtypes, FUSED_GAUSSIAN_HMM = False -- goes through
the plain-torch sequential filter of this file, differentiated by autograd.

GammaGaussianHMM: that model with one Gamma-distributed precision multiplier shared by all its noise, a jointly
Student-t series (reference: pyro/distributions/hmm.py:744-940).  log_prob is ONE launch of the Student-t variant of
the same kernel (pa_gamma_gaussian_hmm_fwd_bwd): the filter at unit scale, then the adjoint sweep at covariances
divided by the series' weight; the routing and the torch route are GaussianHMM's.

LinearHMM: the same linear model with arbitrary reparameterisable noise and optional observation transforms
(reference: pyro/distributions/hmm.py:939-1138).  It has no log_prob; rsample is the reference's Python loop over T
of small batched matmuls (_linear_integrate, hmm.py:32-48), here ONE launch with one lane per sample path
(pa_linear_hmm_draw) when nothing needs a gradient, and that loop in torch ops otherwise.  IndependentHMM: the
reference's wrapper that reads a batch of univariate HMMs as one multivariate one (hmm.py:1141-1198).
"""
import math

import torch

from torch.distributions import constraints

from .base import TorchDistribution


class DiscreteHMM(TorchDistribution):
    arg_constraints = {"initial_logits": constraints.real, "transition_logits": constraints.real}
    has_rsample = False

    def __init__(self, initial_logits, transition_logits, observation_dist, validate_args=None,
                 duration=None):
        if initial_logits.dim() < 1:
            raise ValueError("expected initial_logits to have at least one dim, actual shape = {}"
                             .format(initial_logits.shape))
        if transition_logits.dim() < 2:
            raise ValueError("expected transition_logits to have at least two dims, actual shape = {}"
                             .format(transition_logits.shape))
        if len(observation_dist.batch_shape) < 1:
            raise ValueError("expected observation_dist to have at least one batch dim, actual "
                             ".batch_shape = {}".format(observation_dist.batch_shape))
        shape = torch.broadcast_shapes(initial_logits.shape[:-1] + (1,), transition_logits.shape[:-2],
                                       observation_dist.batch_shape[:-1])
        batch_shape, time_shape = shape[:-1], shape[-1:]
        if duration is not None and time_shape[0] not in (1, duration):
            raise ValueError("duration {} does not match the time axis of size {}".format(
                duration, time_shape[0]))
        event_shape = time_shape + observation_dist.event_shape
        self.initial_logits = initial_logits - initial_logits.logsumexp(-1, True)
        self.transition_logits = transition_logits - transition_logits.logsumexp(-1, True)
        self.observation_dist = observation_dist
        self.duration = duration
        super().__init__(torch.Size(batch_shape), torch.Size(event_shape), validate_args=validate_args)

    @constraints.dependent_property(event_dim=2)
    def support(self):
        return constraints.independent(self.observation_dist.support, 1)

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(DiscreteHMM, _instance)
        batch_shape = torch.Size(torch.broadcast_shapes(self.batch_shape, tuple(batch_shape)))
        # the batch shape is the broadcast of all three inputs: expanding one of them is enough
        new.initial_logits = self.initial_logits.expand(batch_shape + (-1,))
        new.transition_logits = self.transition_logits
        new.observation_dist = self.observation_dist
        new.duration = self.duration
        super(DiscreteHMM, new).__init__(batch_shape, self.event_shape, validate_args=False)
        new._validate_args = self.__dict__.get("_validate_args")
        return new

    def _validate_sample(self, value):
        pass        # time may be longer than event_shape[0] for time-homogeneous parameters

    def _potentials(self, value):
        """(obs_logits [..., T, K], transition logits [..., T | 1, K, K], initial logits, batch shape) of ``value``."""
        from .. import kernels
        obs = self.observation_dist
        value = value.unsqueeze(-1 - len(obs.event_shape))
        obs_logits = obs.log_prob(value)                              # [..., T, K]
        T, K = obs_logits.shape[-2:]
        trans, init = self.transition_logits, self.initial_logits
        if trans.dim() == 2:                       # [K, K]: shared by every step and batch element
            trans = trans.unsqueeze(0)
        batch = torch.broadcast_shapes(init.shape[:-1], trans.shape[:-3], obs_logits.shape[:-2])
        if trans.shape[-3] not in (1, T):
            raise ValueError("transition_logits has {} time steps, the data {}".format(
                trans.shape[-3], T))
        if not kernels.on_device(obs_logits):
            raise RuntimeError("pyro_amd: DiscreteHMM.log_prob needs device tensors (there is no "
                               "CPU implementation in this package)")
        return obs_logits, trans, init, batch

    @staticmethod
    def _forward_recursion(obs_logits, trans, init):
        """More than 64 states (or a dtype the kernel does not take): the forward recursion step by step with
        device tensor ops -> the unnormalised log filtering distribution of the last state."""
        a = init
        for t in range(obs_logits.shape[-2]):
            tr = trans[..., t if trans.shape[-3] > 1 else 0, :, :]
            a = torch.logsumexp(a.unsqueeze(-1) + tr, dim=-2) + obs_logits[..., t, :]
        return a

    @staticmethod
    def _chain_inputs(obs_logits, trans, init, batch):
        """The potentials as the chain kernels take them: unary [B, T + 1, K], pairwise [B, T, K, K] / [T, K, K] /
        [K, K]."""
        T, K = obs_logits.shape[-2:]
        B = 1
        for n in batch:
            B *= int(n)
        unary = torch.cat([init.expand(batch + (K,)).unsqueeze(-2),
                           obs_logits.expand(batch + (T, K))], dim=-2).reshape(B, T + 1, K).contiguous()
        lead = trans.shape[:-3]
        if all(n == 1 for n in lead):                 # shared by the batch: [K, K] or [T, K, K]
            pair = trans.reshape(trans.shape[-3:])
            pair = pair[0].contiguous() if pair.shape[0] == 1 else pair.contiguous()
        else:
            pair = trans.expand(batch + (T, K, K)).reshape(B, T, K, K).contiguous()
        return unary, pair

    def log_prob(self, value):
        from ..ops.contract import _LogChain
        obs_logits, trans, init, batch = self._potentials(value)
        K = obs_logits.shape[-1]
        fused = K <= 64 and obs_logits.dtype in (torch.float32, torch.float64)
        if not fused:
            return torch.logsumexp(self._forward_recursion(obs_logits, trans, init), dim=-1)
        unary, pair = self._chain_inputs(obs_logits, trans, init, batch)
        return _LogChain.invoke(unary, pair).reshape(batch)

    def filter(self, value):
        """The posterior over the final state given the observations ``value``, a ``Categorical`` of batch shape
        ``batch_shape`` (reference: hmm.py:373-394).  It costs nothing new: the chain kernel's gradient with respect
        to the last unary potential IS that posterior.  Detached from the parameters."""
        from .. import kernels
        from . import Categorical
        with torch.no_grad():
            obs_logits, trans, init, batch = self._potentials(value)
            K = obs_logits.shape[-1]
            if K <= 64 and obs_logits.dtype in (torch.float32, torch.float64):
                unary, pair = self._chain_inputs(obs_logits, trans, init, batch)
                _, g_u, _ = kernels.logchain_fwd_bwd(unary, pair)
                return Categorical(probs=g_u[:, -1, :].reshape(batch + (K,)), validate_args=self._validate_args)
            a = self._forward_recursion(obs_logits, trans, init)
            return Categorical(logits=a.expand(batch + (K,)), validate_args=self._validate_args)

    def sample(self, sample_shape=torch.Size()):
        raise NotImplementedError("DiscreteHMM.sample is not built in this backend (log_prob only)")


# ---- GaussianHMM -------------------------------------------------------------------------------------------------
FUSED_GAUSSIAN_HMM = True     # device tensors within the kernel's limits go through pa_gaussian_hmm_fwd_bwd


def _loc_cov(dist, what):
    """(loc, covariance) of a MultivariateNormal or an Independent(Normal, 1), formed differentiably from the
    tensors the caller parametrised it with."""
    td = torch.distributions
    if isinstance(dist, td.MultivariateNormal):
        if "covariance_matrix" in dist.__dict__:
            return dist.loc, dist.covariance_matrix
        # (from precision_matrix: torch forms it differentiably; only the lower triangle counts, as for torch)
        L = dist._unbroadcasted_scale_tril.tril()
        cov = L @ L.transpose(-1, -2)
        return dist.loc, cov.expand(dist.batch_shape + cov.shape[-2:])
    if (isinstance(dist, td.Independent) and dist.reinterpreted_batch_ndims == 1
            and isinstance(dist.base_dist, td.Normal)):
        base = dist.base_dist
        return base.loc, torch.diag_embed(base.scale * base.scale)
    raise ValueError("{} must be a MultivariateNormal or an Independent(Normal, 1), got {}".format(
        what, type(dist).__name__))


def _step(p, t, nd):
    """Step ``t`` of a parameter whose time axis sits ``nd`` dims from the right (size 1: time-homogeneous)."""
    return p.select(-nd - 1, t if p.shape[-nd - 1] > 1 else 0)


def _kalman_steps(m0, P0, F, q, Q, H, r, R, x):
    """The sequential filter in plain torch ops, step by step: parameters broadcastable to [..., T | 1, ...] (m0, P0
    without the time axis), x [..., T, obs]; yields per step (|L^-1 y|^2, sum log diag L, m_t, P_t, whether S had a
    non-positive pivot).  The same arithmetic as csrc/gaussian_hmm.h: P^p symmetrised, S = L L^T, U = P^p H L^-T,
    P = P^p - U U^T."""
    T = x.shape[-2]
    m, P = m0, P0
    for t in range(T):
        Ft, qt, Qt = _step(F, t, 2), _step(q, t, 1), _step(Q, t, 2)
        Ht, rt, Rt = _step(H, t, 2), _step(r, t, 1), _step(R, t, 2)
        mp = (m.unsqueeze(-2) @ Ft).squeeze(-2) + qt
        Pp = Ft.transpose(-1, -2) @ P @ Ft + Qt
        Pp = 0.5 * (Pp + Pp.transpose(-1, -2))
        y = x[..., t, :] - (mp.unsqueeze(-2) @ Ht).squeeze(-2) - rt
        PH = Pp @ Ht
        S = Ht.transpose(-1, -2) @ PH + Rt
        L, info = torch.linalg.cholesky_ex(S)
        batch = torch.broadcast_shapes(L.shape[:-2], y.shape[:-1], PH.shape[:-2])
        L = L.expand(batch + L.shape[-2:])
        v = torch.linalg.solve_triangular(L, y.expand(batch + y.shape[-1:]).unsqueeze(-1), upper=False)
        U = torch.linalg.solve_triangular(L, PH.expand(batch + PH.shape[-2:]).transpose(-1, -2),
                                          upper=False).transpose(-1, -2)
        m = mp + (U @ v).squeeze(-1)
        P = Pp - U @ U.transpose(-1, -2)
        yield v.squeeze(-1).pow(2).sum(-1), L.diagonal(dim1=-2, dim2=-1).log().sum(-1), m, P, info > 0


def _kalman_filter(m0, P0, F, q, Q, H, r, R, x, keep=None):
    """_kalman_steps -> (log_prob [...], filtered mean and covariance of the last state).  A step whose S is not
    positive definite makes the element NaN.  ``keep``: a list that receives every step's (m_t, P_t)."""
    o = x.shape[-1]
    lp, bad = 0.0, False
    for quad, logdet, m, P, info in _kalman_steps(m0, P0, F, q, Q, H, r, R, x):
        bad = info | bad
        lp = lp - 0.5 * quad - logdet - 0.5 * o * math.log(2 * math.pi)
        if keep is not None:
            keep.append((m, P))
    nan = lp.new_full((), float("nan"))
    return torch.where(bad, nan, lp), m, P


def _kalman_terms(m0, P0, F, q, Q, H, r, R, x):
    """_kalman_steps -> (quad = sum_t |L_t^-1 y_t|^2, logdet = sum_t sum log diag L_t, filtered mean and covariance
    of the last state): the two halves of the Gaussian log_prob kept apart, what GammaGaussianHMM needs of the filter
    at unit scale.  NaN (quad and logdet) where a step's S is not positive definite."""
    quad, logdet, bad = 0.0, 0.0, False
    for v2, ld, m, P, info in _kalman_steps(m0, P0, F, q, Q, H, r, R, x):
        bad = info | bad
        quad, logdet = quad + v2, logdet + ld
    nan = quad.new_full((), float("nan"))
    return torch.where(bad, nan, quad), torch.where(bad, nan, logdet), m, P


def _student_log_prob(a, b, quad, logdet, n):
    """log p(x) of the series when every covariance of the model is divided by s ~ Gamma(a, b): the unit-scale
    filter's ``quad`` and ``logdet`` over n = T * obs_dim observed numbers, s integrated out."""
    return (torch.lgamma(a + 0.5 * n) - torch.lgamma(a) + a * b.log() - (a + 0.5 * n) * (b + 0.5 * quad).log()
            - logdet - 0.5 * n * math.log(2 * math.pi))


def _backward_sample_maps(m0, P0, F, q, Q, H, r, R, x):
    """The posterior of the path z_1..z_T given x as a chain run backward, in plain torch ops and with the states
    written as columns: z_T = c_T + L_T eps_T, z_{t-1} = c_{t-1} + G_{t-1} z_t + L_{t-1} eps_{t-1}.  Arguments as
    for _kalman_filter -> (c [..., T, h], G [..., T, h, h] with G_T = 0, L [..., T, h, h] lower triangular).  The
    same arithmetic as csrc/gaussian_hmm_sample.hip: the filter above keeps (m_t, P_t); L_T = chol(sym(P_T)); for
    t = T..2, with m^p, P^p predicted from (m_{t-1}, P_{t-1}) as the filter does,
        G = P_{t-1} F (P^p)^-1,   c_{t-1} = m_{t-1} - G m^p,   J = I - G F^T,
        L_{t-1} = chol(sym(J P_{t-1} J^T + G Q G^T))
    -- the conditional covariance in Joseph form, a sum of two positive semi-definite terms: P_{t-1} - G P^p G^T
    loses positive definiteness in float32 when Q is nearly singular.  An element with a non-positive pivot, in the
    filter or in a factor here, is NaN throughout."""
    T = x.shape[-2]
    kept = []
    lp, _, _ = _kalman_filter(m0, P0, F, q, Q, H, r, R, x, keep=kept)
    bad = torch.isnan(lp)
    batch = lp.shape
    m, P = kept[-1]
    h = m.shape[-1]
    L, info = torch.linalg.cholesky_ex(0.5 * (P + P.transpose(-1, -2)))
    bad = (info > 0) | bad
    eye = torch.eye(h, dtype=m.dtype, device=m.device)
    cs, Gs, Ls = [m.expand(batch + (h,))], [torch.zeros_like(P).expand(batch + (h, h))], [L.expand(batch + (h, h))]
    for t in range(T - 1, 0, -1):
        m, P = kept[t - 1]
        Ft, qt, Qt = _step(F, t, 2), _step(q, t, 1), _step(Q, t, 2)
        mp = (m.unsqueeze(-2) @ Ft).squeeze(-2) + qt
        FtP = Ft.transpose(-1, -2) @ P
        Pp = FtP @ Ft + Qt
        Pp = 0.5 * (Pp + Pp.transpose(-1, -2))
        Lp, info = torch.linalg.cholesky_ex(Pp)
        bad = (info > 0) | bad
        G = torch.cholesky_solve(FtP, Lp).transpose(-1, -2)
        J = eye - G @ Ft.transpose(-1, -2)
        C = (J @ P) @ J.transpose(-1, -2) + (G @ Qt) @ G.transpose(-1, -2)
        L, info = torch.linalg.cholesky_ex(0.5 * (C + C.transpose(-1, -2)))
        bad = (info > 0) | bad
        cs.append((m - (G @ mp.unsqueeze(-1)).squeeze(-1)).expand(batch + (h,)))
        Gs.append(G.expand(batch + (h, h)))
        Ls.append(L.expand(batch + (h, h)))
    c, G, L = (torch.stack(v[::-1], dim=len(batch)) for v in (cs, Gs, Ls))
    nan = c.new_full((), float("nan"))
    return (torch.where(bad[..., None, None], nan, c), torch.where(bad[..., None, None, None], nan, G),
            torch.where(bad[..., None, None, None], nan, L))


def _backward_sample(c, G, L, eps):
    """The paths [..., T, h] of the maps for the standard normal ``eps`` [sample_shape, ..., T, h]."""
    T = eps.shape[-2]
    z, out = None, []
    for t in range(T - 1, -1, -1):
        zt = c[..., t, :] + (L[..., t, :, :] @ eps[..., t, :, None]).squeeze(-1)
        if z is not None:
            zt = zt + (G[..., t, :, :] @ z.unsqueeze(-1)).squeeze(-1)
        z = zt
        out.append(z)
    return torch.stack(out[::-1], dim=-2)


def _rts_smoother(m0, P0, F, q, Q, H, r, R, x):
    """The smoothed marginals of z_1..z_T given x in plain torch ops, with the states written as columns.  Arguments
    as for _kalman_filter -> (mean [..., T, h], cov [..., T, h, h], cross [..., T - 1, h, h] with cross_t =
    Cov(z_t, z_{t+1} | x), rows z_t).  The same arithmetic as csrc/gaussian_hmm_smooth.hip: the filter above keeps
    (m_t, P_t); ms_T = m_T, Ps_T = sym(P_T); for t = T..2, with m^p, P^p predicted from (m_{t-1}, P_{t-1}) as the
    filter does and P^p = L L^T,
        G = P_{t-1} F (P^p)^-1,   cross_{t-1} = G Ps_t,   ms_{t-1} = m_{t-1} + G (ms_t - m^p),
        Ps_{t-1} = sym(P_{t-1} + (G (Ps_t - P^p)) G^T)
    -- the subtraction form: nothing is factorised from Ps, so it need not stay positive definite for the recursion
    to go on, and in float32 it is as accurate as the Joseph form of _backward_sample_maps or better.  An element
    with a non-positive pivot, in the filter, in a factor of P^p or in the Q_t of a step the sweep visits (t = 2..T;
    checked for its pivots alone, as the kernel does: F^T P F + Q is often positive definite where Q is not), is NaN
    throughout.  P0 is never checked.  Differentiable."""
    T = x.shape[-2]
    kept = []
    lp, _, _ = _kalman_filter(m0, P0, F, q, Q, H, r, R, x, keep=kept)
    bad = torch.isnan(lp)
    batch = lp.shape
    m, P = kept[-1]
    h = m.shape[-1]
    ms, Ps = m, 0.5 * (P + P.transpose(-1, -2))
    means, covs, crosses = [ms.expand(batch + (h,))], [Ps.expand(batch + (h, h))], []
    for t in range(T - 1, 0, -1):
        m, P = kept[t - 1]
        Ft, qt, Qt = _step(F, t, 2), _step(q, t, 1), _step(Q, t, 2)
        mp = (m.unsqueeze(-2) @ Ft).squeeze(-2) + qt
        FtP = Ft.transpose(-1, -2) @ P
        Pp = FtP @ Ft + Qt
        Pp = 0.5 * (Pp + Pp.transpose(-1, -2))
        Lp, info = torch.linalg.cholesky_ex(Pp)
        bad = (info > 0) | (torch.linalg.cholesky_ex(Qt)[1] > 0) | bad          # (Q_t: for its pivots alone)
        G = torch.cholesky_solve(FtP, Lp).transpose(-1, -2)
        crosses.append((G @ Ps).expand(batch + (h, h)))
        ms = m + (G @ (ms - mp).unsqueeze(-1)).squeeze(-1)
        Ps = P + (G @ (Ps - Pp)) @ G.transpose(-1, -2)
        Ps = 0.5 * (Ps + Ps.transpose(-1, -2))
        means.append(ms.expand(batch + (h,)))
        covs.append(Ps.expand(batch + (h, h)))
    mean, cov = (torch.stack(v[::-1], dim=len(batch)) for v in (means, covs))
    cross = torch.stack(crosses[::-1], dim=len(batch)) if crosses else cov.new_zeros(batch + (0, h, h))
    nan = mean.new_full((), float("nan"))
    return (torch.where(bad[..., None, None], nan, mean), torch.where(bad[..., None, None, None], nan, cov),
            torch.where(bad[..., None, None, None], nan, cross))


class GaussianHMM(TorchDistribution):
    """Hidden Markov model with Gaussian initial, transition and observation distributions (reference:
    pyro/distributions/hmm.py:434-741), the generative model

        z = initial_dist.sample()
        for t in range(num_steps):
            z = z @ transition_matrix + transition_dist.sample()
            x[t] = z @ observation_matrix + observation_dist.sample()

    with ``event_shape = (num_steps, obs_dim)``; time-homogeneous parameters give ``num_steps = 1`` and take data of
    any length.  Each of the three distributions is a ``MultivariateNormal`` or an ``Independent(Normal, 1)``
    (this package's classes or torch's).

    ``log_prob`` is differentiable in every parameter and in the value.  Device tensors in float32 / float64 with
    hidden and obs dimension up to 16 take ONE launch of the Kalman filter / smoother kernel; everything else (CPU
    tensors, larger dimensions, other dtypes, ``hmm.FUSED_GAUSSIAN_HMM = False``) the sequential torch filter of
    this module.

    ``rsample_posterior`` draws the whole latent path given the data: two launches (csrc/gaussian_hmm_sample.hip) for
    the same tensors when nothing needs a gradient, the backward-sampling loop of this module otherwise.

    ``smooth`` gives the smoothed marginals of every latent state given all the data -- mean, covariance and the
    lag-one cross covariance: ONE launch (csrc/gaussian_hmm_smooth.hip) for the same tensors when nothing needs a
    gradient, the Rauch-Tung-Striebel loop of this module, differentiable, otherwise.

    ``rsample`` draws sample paths of the observations, and with ``prefix_condition(data).rsample(...)`` forecasts:
    again two launches (csrc/gaussian_hmm_draw.hip) for the same tensors when nothing needs a gradient, after the
    filter's one launch for a forecast; the generative loop in torch ops, reparameterised, otherwise.

    ``LinearHMM`` (arbitrary noise, no ``log_prob``) and ``IndependentHMM`` are below; ``infer.reparam`` has
    ``LinearHMMReparam`` and ``StudentTReparam``, which turn a heavy-tailed ``LinearHMM`` site into this class with
    per-step diagonal covariances.  Not built here: ``conjugate_update``, ``GaussianMRF``, ``Stable`` and its
    reparameterisers, and missing observations."""
    arg_constraints = {}
    has_rsample = True
    support = constraints.independent(constraints.real, 2)

    def __init__(self, initial_dist, transition_matrix, transition_dist, observation_matrix, observation_dist,
                 validate_args=None, duration=None):
        if not isinstance(transition_matrix, torch.Tensor) or transition_matrix.dim() < 2:
            raise ValueError("transition_matrix must be a tensor [..., hidden_dim, hidden_dim]")
        if not isinstance(observation_matrix, torch.Tensor) or observation_matrix.dim() < 2:
            raise ValueError("observation_matrix must be a tensor [..., hidden_dim, obs_dim]")
        m0, P0 = _loc_cov(initial_dist, "initial_dist")
        q, Q = _loc_cov(transition_dist, "transition_dist")
        r, R = _loc_cov(observation_dist, "observation_dist")
        hidden_dim, obs_dim = observation_matrix.shape[-2:]
        if initial_dist.event_shape != (hidden_dim,) or transition_dist.event_shape != (hidden_dim,) \
                or transition_matrix.shape[-2:] != (hidden_dim, hidden_dim) \
                or observation_dist.event_shape != (obs_dim,):
            raise ValueError("expected initial_dist and transition_dist over {0} dims, transition_matrix "
                             "[..., {0}, {0}] and observation_dist over {1} dims".format(hidden_dim, obs_dim))
        # a time axis on everything but the initial state (batch shape () = shared and time-homogeneous)
        m0 = m0.expand(initial_dist.batch_shape + (hidden_dim,))
        P0 = P0.expand(initial_dist.batch_shape + (hidden_dim, hidden_dim))
        F = transition_matrix if transition_matrix.dim() > 2 else transition_matrix.unsqueeze(0)
        H = observation_matrix if observation_matrix.dim() > 2 else observation_matrix.unsqueeze(0)
        tb = transition_dist.batch_shape or (1,)
        ob = observation_dist.batch_shape or (1,)
        q, Q = q.expand(tb + (hidden_dim,)), Q.expand(tb + (hidden_dim, hidden_dim))
        r, R = r.expand(ob + (obs_dim,)), R.expand(ob + (obs_dim, obs_dim))
        self._setup(m0, P0, F, q, Q, H, r, R, duration, validate_args)

    def _setup(self, m0, P0, F, q, Q, H, r, R, duration, validate_args):
        hidden_dim, obs_dim = H.shape[-2:]
        shape = torch.broadcast_shapes(m0.shape[:-1] + (1,), F.shape[:-2], q.shape[:-1], H.shape[:-2], r.shape[:-1])
        batch_shape, time_shape = shape[:-1], shape[-1:]
        if duration is not None and time_shape[0] not in (1, duration):
            raise ValueError("duration {} does not match the time axis of size {}".format(duration, time_shape[0]))
        if duration is None and time_shape[0] != 1:
            duration = time_shape[0]
        self.hidden_dim, self.obs_dim, self.duration = hidden_dim, obs_dim, duration
        self._parts = (m0, P0, F, q, Q, H, r, R)
        super().__init__(torch.Size(batch_shape), torch.Size(time_shape + (obs_dim,)), validate_args=validate_args)

    @classmethod
    def _from_parts(cls, parts, duration, validate_args):
        new = cls.__new__(cls)
        new._setup(*parts, duration, validate_args)
        return new

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(GaussianHMM, _instance)
        batch_shape = torch.Size(torch.broadcast_shapes(self.batch_shape, tuple(batch_shape)))
        m0, P0 = self._parts[:2]
        # the batch shape is the broadcast of all the parts: expanding the initial state is enough
        new._parts = (m0.expand(batch_shape + m0.shape[-1:]), P0.expand(batch_shape + P0.shape[-2:])) + self._parts[2:]
        new.hidden_dim, new.obs_dim, new.duration = self.hidden_dim, self.obs_dim, self.duration
        super(GaussianHMM, new).__init__(batch_shape, self.event_shape, validate_args=False)
        new._validate_args = self.__dict__.get("_validate_args")
        return new

    def _validate_sample(self, value):
        pass        # time may be longer than event_shape[0] for time-homogeneous parameters

    def _check_value(self, value):
        if value.dim() < 2 or value.shape[-1] != self.obs_dim:
            raise ValueError("expected a value [..., num_steps, {}], got {}".format(self.obs_dim, tuple(value.shape)))
        T = value.shape[-2]
        for p, nd in zip(self._parts[2:], (2, 1, 2, 2, 1, 2)):
            if p.shape[-nd - 1] not in (1, T):
                raise ValueError("a parameter has {} time steps, the data {}".format(p.shape[-nd - 1], T))
        return torch.broadcast_shapes(self.batch_shape, value.shape[:-2]), T

    def _takes_kernel(self, value):
        from .. import kernels
        return (FUSED_GAUSSIAN_HMM and value.dtype in (torch.float32, torch.float64)
                and all(kernels.on_device(t) and t.dtype == value.dtype for t in self._parts + (value,))
                and self.hidden_dim <= kernels.GAUSSIAN_HMM_MAX_HIDDEN
                and self.obs_dim <= kernels.GAUSSIAN_HMM_MAX_OBS)

    def _kernel_inputs(self, value, batch, T):
        """The parts as _kernel_parts lays them out, then the data [B, T, obs_dim]."""
        B = 1
        for n in batch:
            B *= int(n)
        value = value.expand(batch + (T, self.obs_dim)).reshape(B, T, self.obs_dim).contiguous()
        return self._kernel_parts(batch) + [value]

    def _kernel_parts(self, batch):
        """The parts in the layouts of kernels.gaussian_hmm_fwd_bwd: a parameter whose batch dims are all 1 or all
        expanded (stride 0: what broadcasting a shared location against a per-sequence scale leaves behind) stays
        shared ([1, ...], batch stride 0), any other is expanded to the B sequences; the time axis keeps its size."""
        B = 1
        for n in batch:
            B *= int(n)
        out = []
        for i, (p, nd) in enumerate(zip(self._parts, (1, 2, 2, 1, 2, 2, 1, 2))):
            tail = p.shape[-nd - (1 if i >= 2 else 0):]
            lead = p.shape[:p.dim() - len(tail)]
            if all(n == 1 or (n > 1 and s == 0) for n, s in zip(lead, p.stride())):
                out.append(p[(0,) * len(lead)].reshape((1,) + tuple(tail)).contiguous())
            else:
                out.append(p.expand(batch + tuple(tail)).reshape((B,) + tuple(tail)).contiguous())
        return out

    def log_prob(self, value):
        batch, T = self._check_value(value)
        if self._takes_kernel(value):
            from ..ops.contract import _GaussianHMM
            return _GaussianHMM.invoke(*self._kernel_inputs(value, batch, T)).reshape(batch)
        lp, _, _ = _kalman_filter(*self._parts, value)
        return lp.expand(batch)

    def filter(self, value):
        """The posterior over the final state given the observations ``value``: a ``MultivariateNormal`` of batch
        shape ``batch_shape`` that can serve as the ``initial_dist`` of a model of what follows.  It comes from the
        forward pass alone and is DETACHED from the parameters (the reference's is differentiable)."""
        from . import MultivariateNormal
        batch, T = self._check_value(value)
        with torch.no_grad():
            if self._takes_kernel(value):
                from .. import kernels
                args = [t.detach() for t in self._kernel_inputs(value, batch, T)]
                _, (m, P), _ = kernels.gaussian_hmm_fwd_bwd(*args, need_grads=False, need_filter=True)
                m, P = m.reshape(batch + m.shape[-1:]), P.reshape(batch + P.shape[-2:])
            else:
                _, m, P = _kalman_filter(*self._parts, value)
                m, P = m.expand(batch + m.shape[-1:]), P.expand(batch + P.shape[-2:])
                P = 0.5 * (P + P.transpose(-1, -2))
        return MultivariateNormal(m, covariance_matrix=P, validate_args=self._validate_args)

    def rsample_posterior(self, value, sample_shape=torch.Size(), *, noise=None):
        """Draws of the latent path ``z_1..z_T`` given the observations ``value`` [..., T, obs_dim] (reference:
        hmm.py:596-604): a tensor of shape ``sample_shape + batch + (T, hidden_dim)`` with ``batch`` the broadcast of
        ``batch_shape`` and ``value.shape[:-2]``.  The initial state ``z_0`` is not drawn, as in the reference.

        ``noise``: standard normal of the output's shape; drawn with ``torch.randn`` on the parameters' device when
        not given, so ``torch.manual_seed`` reproduces a call; zeros give the posterior mean.  (The reference's
        method has no such argument, its ops function does.)  The map from noise to path is this package's:
        sequential, ``z_T`` first and every earlier state given the next one, over T rows of noise -- not the
        reference's parallel scan over T + 1 rows.  The distribution of the paths is the same.

        With grad mode on and a parameter, ``value`` or ``noise`` requiring a gradient the draws are reparameterised:
        the torch route, differentiable in all of them (it also serves CPU tensors, dimensions over 16, other dtypes
        and ``hmm.FUSED_GAUSSIAN_HMM = False``).  Otherwise device tensors within the kernel's limits take the two
        launches of csrc/gaussian_hmm_sample.hip and the result is DETACHED, like ``filter``'s.  A series with a
        non-positive pivot has NaN paths."""
        batch, T = self._check_value(value)
        shape = torch.Size(sample_shape) + batch + (T, self.hidden_dim)
        if noise is None:
            noise = torch.randn(shape, dtype=value.dtype, device=self._parts[0].device)
        elif noise.shape != shape:
            raise ValueError("expected noise of shape {}, got {}".format(tuple(shape), tuple(noise.shape)))
        tensors = self._parts + (value, noise)
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
        from .. import kernels
        if (not needs_grad and self._takes_kernel(value) and kernels.on_device(noise)
                and noise.dtype == value.dtype):
            args = [t.detach() for t in self._kernel_inputs(value, batch, T)]
            eps = noise.detach().reshape((-1,) + tuple(args[-1].shape[:2]) + (self.hidden_dim,)).contiguous()
            z, _ = kernels.gaussian_hmm_sample(*args, eps)
            return z.reshape(shape)
        c, G, L = _backward_sample_maps(*self._parts, value)
        return _backward_sample(c, G, L, noise).expand(shape)

    def smooth(self, value, cross=False):
        """The smoothed marginals of the latent states given ALL the observations ``value`` [..., T, obs_dim]:
        ``(mean, cov)`` with ``mean[..., t, :] = E[z_t | x_1..T]`` of shape ``batch + (T, hidden_dim)`` and
        ``cov[..., t, :, :] = Cov[z_t | x_1..T]`` of shape ``batch + (T, hidden_dim, hidden_dim)``, ``batch`` the
        broadcast of ``batch_shape`` and ``value.shape[:-2]``; with ``cross=True`` ``(mean, cov, cross)``, where
        ``cross[..., t, :, :] = Cov[z_t, z_{t+1} | x_1..T]`` (rows ``z_t``, columns ``z_{t+1}``) has shape
        ``batch + (T - 1, hidden_dim, hidden_dim)``.  The initial state ``z_0`` is not included, as in
        ``rsample_posterior``.  These are a state estimate with its error band, and the E-step of EM.  (The
        reference's class has no such method.)

        The Rauch-Tung-Striebel recursion after the Kalman filter: ``ms_T = m_T``, ``Ps_T = sym(P_T)`` and, with the
        states as columns, ``G = P_{t-1} F (P^p)^-1``, ``ms_{t-1} = m_{t-1} + G (ms_t - m^p)``,
        ``Ps_{t-1} = sym(P_{t-1} + G (Ps_t - P^p) G^T)``, ``cross_{t-1} = G Ps_t``.

        The routing is ``rsample_posterior``'s.  With grad mode on and a parameter or ``value`` requiring a gradient:
        the torch route, differentiable in all of them (it also serves CPU tensors, dimensions over 16, other dtypes
        and ``hmm.FUSED_GAUSSIAN_HMM = False``).  Otherwise device tensors within the kernel's limits take the ONE
        launch of csrc/gaussian_hmm_smooth.hip and the result is DETACHED, like ``filter``'s.  A series with a
        non-positive pivot, of the filter, of a predicted covariance or of a transition covariance the backward sweep
        uses (steps 2..T), is NaN in all three."""
        batch, T = self._check_value(value)
        h = self.hidden_dim
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in self._parts + (value,))
        shapes = (batch + (T, h), batch + (T, h, h), batch + (T - 1, h, h))[:3 if cross else 2]
        if not needs_grad and self._takes_kernel(value):
            from .. import kernels
            args = [t.detach() for t in self._kernel_inputs(value, batch, T)]
            out = kernels.gaussian_hmm_smooth(*args, need_cross=cross)
            return tuple(v.reshape(s) for v, s in zip(out, shapes))
        return tuple(v.expand(s) for v, s in zip(_rts_smoother(*self._parts, value), shapes))

    def prefix_condition(self, data):
        """Given ``event_shape == (t + f, d)`` and ``data`` [..., t, d], the conditional distribution of the
        remaining ``f`` steps (reference: hmm.py:690-741): ``filter(data)`` under the first ``t`` steps' parameters
        becomes the initial distribution of the other ``f``."""
        if self.duration is None:
            raise ValueError("prefix_condition needs a duration")
        if data.dim() < 2 or data.size(-1) != self.obs_dim or not data.size(-2) < self.duration:
            raise ValueError("expected data [..., t < {}, {}], got {}".format(self.duration, self.obs_dim,
                                                                              tuple(data.shape)))
        t = data.size(-2)
        f = self.duration - t
        left, right = [], []
        for p, nd in zip(self._parts[2:], (2, 1, 2, 2, 1, 2)):
            hom = p.shape[-nd - 1] == 1
            left.append(p if hom else p.narrow(-nd - 1, 0, t))
            right.append(p if hom else p.narrow(-nd - 1, t, f))
        post = GaussianHMM._from_parts(self._parts[:2] + tuple(left), t, self._validate_args).filter(data)
        return GaussianHMM._from_parts((post.loc, post.covariance_matrix) + tuple(right), f, self._validate_args)

    def rsample(self, sample_shape=torch.Size(), *, noise=None):
        """Sample paths of the observations, ``sample_shape + batch_shape + (duration, obs_dim)`` (reference:
        hmm.py:584-594); needs ``duration``.  With ``L L^T`` the Cholesky factors of the three covariances

            z_0 = m0 + L_0 e_0,   z_t = z_{t-1} F_t + q_t + L_{Q,t} e_t,   x_t = z_t H_t + r_t + L_{R,t} e'_t

        ``noise``: the triple ``(e_0, e, e')`` of standard normals of shapes ``sample_shape + batch_shape`` +
        ``(hidden_dim,)``, ``(duration, hidden_dim)`` and ``(duration, obs_dim)``; zeros give the mean path.  (The
        keyword is this package's, as for ``rsample_posterior``.)

        Device tensors in float32 / float64 within the kernels' limits, with nothing requiring a gradient under grad
        mode, take the two launches of csrc/gaussian_hmm_draw.hip and the result is DETACHED.  Noise that is not given
        is then ONE ``torch.randn`` of the total size on the parameters' device, split into the three arrays, so
        ``torch.manual_seed`` reproduces a call -- but the device draws for a given seed differ from those of the
        torch route (the distribution does not).  A series with a covariance that is not positive definite has NaN
        paths there.

        Everything else -- grad mode with a parameter or the noise requiring a gradient, CPU tensors, dimensions over
        16, other dtypes, ``hmm.FUSED_GAUSSIAN_HMM = False`` -- is the generative loop in torch ops: reparameterised
        in every parameter and in the noise, raising where ``torch.linalg.cholesky`` raises, and without ``noise``
        drawing per step exactly as it always has."""
        if self.duration is None:
            raise ValueError("GaussianHMM.rsample needs a duration (time-homogeneous parameters do not tell it)")
        m0, P0, F, q, Q, H, r, R = self._parts
        T, h, o = self.duration, self.hidden_dim, self.obs_dim
        shape = torch.Size(sample_shape) + self.batch_shape
        shapes = (shape + (h,), shape + (T, h), shape + (T, o))
        if noise is not None:
            noise = tuple(noise)
            if len(noise) != 3 or any(e.shape != s for e, s in zip(noise, shapes)):
                raise ValueError("expected noise as a triple of shapes {}, {} and {}, got {}".format(
                    *(tuple(s) for s in shapes), [tuple(e.shape) for e in noise]))
        tensors = self._parts + (noise or ())
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
        from .. import kernels
        if (not needs_grad and FUSED_GAUSSIAN_HMM and m0.dtype in (torch.float32, torch.float64)
                and all(kernels.on_device(t) and t.dtype == m0.dtype for t in tensors)
                and h <= kernels.GAUSSIAN_HMM_MAX_HIDDEN and o <= kernels.GAUSSIAN_HMM_MAX_OBS):
            if noise is None:
                sizes = [s.numel() for s in shapes]
                flat = torch.randn(sum(sizes), dtype=m0.dtype, device=m0.device)
                noise = [e.reshape(s) for e, s in zip(flat.split(sizes), shapes)]
            args = [t.detach() for t in self._kernel_parts(self.batch_shape)]
            B = self.batch_shape.numel()
            eps = [e.detach().reshape((-1, B) + tuple(s[len(shape):])).contiguous() for e, s in zip(noise, shapes)]
            x, _ = kernels.gaussian_hmm_draw(*args, T, *eps)
            return x.reshape(shapes[2])

        def draw(loc, cov, given):
            L = torch.linalg.cholesky(cov)
            eps = torch.randn(shape + loc.shape[-1:], dtype=loc.dtype, device=loc.device) if given is None else given
            return loc + (L @ eps.unsqueeze(-1)).squeeze(-1)

        e0, ez, ex = noise or (None, None, None)
        z = draw(m0, P0, e0)
        xs = []
        for t in range(T):
            z = (z.unsqueeze(-2) @ _step(F, t, 2)).squeeze(-2) \
                + draw(_step(q, t, 1), _step(Q, t, 2), None if ez is None else ez[..., t, :])
            xs.append((z.unsqueeze(-2) @ _step(H, t, 2)).squeeze(-2)
                      + draw(_step(r, t, 1), _step(R, t, 2), None if ex is None else ex[..., t, :]))
        return torch.stack(xs, dim=-2)


# ---- GammaGaussianHMM --------------------------------------------------------------------------------------------
class GammaGaussianHMM(TorchDistribution):
    """Linear state-space model whose initial, process and observation noise share one Gamma-distributed precision
    multiplier, so that the series is jointly multivariate Student-t (reference: pyro/distributions/hmm.py:744-940):

        s = scale_dist.sample()
        z = N(initial_dist.loc, initial_dist.covariance / s).sample()
        for t in range(num_steps):
            z = z @ transition_matrix + N(transition_dist.loc, transition_dist.covariance / s).sample()
            x[t] = z @ observation_matrix + N(observation_dist.loc, observation_dist.covariance / s).sample()

    Argument order and shape rules are the reference's: ``scale_dist`` is a ``Gamma`` (this package's or torch's)
    whose batch shape joins the broadcast of the others', which are those of ``GaussianHMM``; each of the three noise
    distributions is a ``MultivariateNormal`` or an ``Independent(Normal, 1)`` (the reference takes the former only).

    The means, gains and covariance ratios of the Kalman filter do not depend on ``s``, so ONE filter at unit scale
    gives ``quad = sum_t |L_t^-1 y_t|^2`` and ``logdet = sum_t sum log diag L_t`` and, with ``n = T * obs_dim``,

        log_prob = lgamma(a + n/2) - lgamma(a) + a log b - (a + n/2) log(b + quad/2) - logdet - n/2 log(2 pi)

    ``log_prob`` is differentiable in every parameter, in ``concentration`` and ``rate`` and in the value.  Device
    tensors in float32 / float64 with hidden and obs dimension up to 16 take ONE launch of the Student-t variant of
    the Kalman filter kernel (pa_gamma_gaussian_hmm_fwd_bwd: the filter, then the adjoint sweep of the Gaussian
    model at covariances divided by ``w = (a + n/2) / (b + quad/2)``); everything else (CPU tensors, larger
    dimensions, other dtypes, ``hmm.FUSED_GAUSSIAN_HMM = False``) the sequential torch filter of this module.

    ``filter`` gives the posteriors of the multiplier and, at unit scale, of the final state.

    Not built: ``rsample``, and ``smooth`` / ``rsample_posterior`` for this model."""
    arg_constraints = {}
    has_rsample = False
    support = constraints.independent(constraints.real, 2)

    def __init__(self, scale_dist, initial_dist, transition_matrix, transition_dist, observation_matrix,
                 observation_dist, validate_args=None, duration=None):
        if not isinstance(scale_dist, torch.distributions.Gamma):
            raise ValueError("scale_dist must be a Gamma, got {}".format(type(scale_dist).__name__))
        unit = GaussianHMM(initial_dist, transition_matrix, transition_dist, observation_matrix, observation_dist,
                           validate_args=False, duration=duration)
        batch_shape = torch.Size(torch.broadcast_shapes(scale_dist.batch_shape, unit.batch_shape))
        self._setup(scale_dist.concentration, scale_dist.rate, unit, batch_shape, validate_args)

    def _setup(self, concentration, rate, unit, batch_shape, validate_args):
        # (the unit-scale model carries the whole batch shape: its expand touches the initial state alone)
        self._unit = unit if unit.batch_shape == batch_shape else unit.expand(batch_shape)
        self.concentration, self.rate = concentration, rate
        self.hidden_dim, self.obs_dim, self.duration = unit.hidden_dim, unit.obs_dim, unit.duration
        super().__init__(batch_shape, unit.event_shape, validate_args=validate_args)

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(GammaGaussianHMM, _instance)
        batch_shape = torch.Size(torch.broadcast_shapes(self.batch_shape, tuple(batch_shape)))
        new._setup(self.concentration, self.rate, self._unit, batch_shape, False)
        new._validate_args = self.__dict__.get("_validate_args")
        return new

    def _validate_sample(self, value):
        pass        # time may be longer than event_shape[0] for time-homogeneous parameters

    def _takes_kernel(self, value):
        from .. import kernels
        return (self._unit._takes_kernel(value)
                and all(kernels.on_device(t) and t.dtype == value.dtype for t in (self.concentration, self.rate)))

    def _kernel_scale(self, batch):
        """``concentration`` and ``rate`` as kernels.gamma_gaussian_hmm_fwd_bwd takes them: [1] when shared by the
        series (batch stride 0), else [B]."""
        out = []
        for p in (self.concentration, self.rate):
            out.append(p.reshape(1) if p.numel() == 1 else p.expand(batch).reshape(-1).contiguous())
        return out

    def log_prob(self, value):
        batch, T = self._unit._check_value(value)
        if self._takes_kernel(value):
            from ..ops.contract import _GammaGaussianHMM
            return _GammaGaussianHMM.invoke(*self._kernel_scale(batch),
                                            *self._unit._kernel_inputs(value, batch, T)).reshape(batch)
        quad, logdet, _, _ = _kalman_terms(*self._unit._parts, value)
        return _student_log_prob(self.concentration, self.rate, quad, logdet, T * self.obs_dim).expand(batch)

    def filter(self, value):
        """The posteriors given the observations ``value``: ``(Gamma, MultivariateNormal)`` of batch shape
        ``batch_shape`` -- the multiplier's, ``Gamma(a + n/2, b + quad/2)``, and the final state's at unit scale (given
        ``s`` its covariance is the returned one divided by ``s``).  The normal has the filter's ``m_T`` as location
        and the filter's ``P_T`` as COVARIANCE.  (The reference builds its normal with ``scale_tril =
        cholesky(precision)``, so that its ``scale_tril scale_tril^T`` is ``P_T^-1``.)  From the forward pass alone and
        DETACHED from the parameters, as ``GaussianHMM.filter`` is."""
        from . import Gamma, MultivariateNormal
        batch, T = self._unit._check_value(value)
        n = T * self.obs_dim
        with torch.no_grad():
            if self._takes_kernel(value):
                from .. import kernels
                args = [t.detach() for t in self._kernel_scale(batch) + self._unit._kernel_inputs(value, batch, T)]
                quad, _, (m, P), _ = kernels.gamma_gaussian_hmm_fwd_bwd(*args, need_grads=False, need_filter=True)
                quad, m, P = quad.reshape(batch), m.reshape(batch + m.shape[-1:]), P.reshape(batch + P.shape[-2:])
            else:
                quad, _, m, P = _kalman_terms(*self._unit._parts, value)
                m, P = m.expand(batch + m.shape[-1:]), P.expand(batch + P.shape[-2:])
                P = 0.5 * (P + P.transpose(-1, -2))
            a = (self.concentration + 0.5 * n).expand(batch)
            b = (self.rate + 0.5 * quad).expand(batch)
        return (Gamma(a, b, validate_args=self._validate_args),
                MultivariateNormal(m, covariance_matrix=P, validate_args=self._validate_args))


# ---- LinearHMM ---------------------------------------------------------------------------------------------------
FUSED_LINEAR_HMM = True       # device tensors within the kernel's limits go through pa_linear_hmm_draw


def _kernel_matrix(m, nb):
    """A matrix [batch..., T | 1, rows, cols] as kernels.linear_hmm_draw takes it, [B | 1, T | 1, rows, cols]
    contiguous: the eager expansion is undone where it was one (stride 0), so that a shared matrix stays shared and a
    time-homogeneous one is staged once."""
    if all(m.shape[i] == 1 or m.stride(i) == 0 for i in range(nb)):
        m = m[(0,) * nb].unsqueeze(0)
    else:
        m = m.reshape((-1,) + tuple(m.shape[nb:]))
    if m.shape[1] > 1 and m.stride(1) == 0:
        m = m[:, :1]
    return m.contiguous()


class LinearHMM(TorchDistribution):
    """Hidden Markov model with linear dynamics and observations and ARBITRARY reparameterisable noise for the
    initial, transition and observation distributions (reference: pyro/distributions/hmm.py:939-1138), the
    generative model

        z = initial_dist.sample()
        for t in range(num_steps):
            z = z @ transition_matrix + transition_dist.sample()
            y = z @ observation_matrix + obs_base_dist.sample()
            x[t] = obs_transform(y)

    where ``observation_dist`` is split into ``obs_base_dist`` and the transforms peeled off its
    ``TransformedDistribution`` layers.  ``event_shape = (num_steps, obs_dim)``; argument checks and shape rules are
    the reference's: the time axis comes from broadcasting, ``duration`` names it for time-homogeneous parameters,
    everything is expanded eagerly.

    There is no ``log_prob``: train through ``infer.reparam.LinearHMMReparam``, which makes the site a conditionally
    Gaussian ``GaussianHMM``.

    ``rsample`` is ONE launch (csrc/linear_hmm.hip) for device tensors when nothing needs a gradient, the loop in
    torch ops, reparameterised, otherwise."""
    arg_constraints = {}
    has_rsample = True

    def __init__(self, initial_dist, transition_matrix, transition_dist, observation_matrix, observation_dist,
                 validate_args=None, duration=None):
        if not isinstance(transition_matrix, torch.Tensor) or transition_matrix.dim() < 2:
            raise ValueError("transition_matrix must be a tensor [..., hidden_dim, hidden_dim]")
        if not isinstance(observation_matrix, torch.Tensor) or observation_matrix.dim() < 2:
            raise ValueError("observation_matrix must be a tensor [..., hidden_dim, obs_dim]")
        for d, what in ((initial_dist, "initial_dist"), (transition_dist, "transition_dist"),
                        (observation_dist, "observation_dist")):
            if not d.has_rsample or len(d.event_shape) != 1:
                raise ValueError("{} must be reparameterisable with one event dim".format(what))
        hidden_dim, obs_dim = observation_matrix.shape[-2:]
        if initial_dist.event_shape != (hidden_dim,) or transition_dist.event_shape != (hidden_dim,) \
                or transition_matrix.shape[-2:] != (hidden_dim, hidden_dim) \
                or observation_dist.event_shape != (obs_dim,):
            raise ValueError("expected initial_dist and transition_dist over {0} dims, transition_matrix "
                             "[..., {0}, {0}] and observation_dist over {1} dims".format(hidden_dim, obs_dim))
        shape = torch.broadcast_shapes(initial_dist.batch_shape + (1,), transition_matrix.shape[:-2],
                                       transition_dist.batch_shape, observation_matrix.shape[:-2],
                                       observation_dist.batch_shape)
        batch_shape, time_shape = torch.Size(shape[:-1]), torch.Size(shape[-1:])
        event_shape = self._init_duration(duration, time_shape + (obs_dim,))
        super().__init__(batch_shape, event_shape, validate_args=validate_args)

        # expand eagerly
        if initial_dist.batch_shape != batch_shape:
            initial_dist = initial_dist.expand(batch_shape)
        if transition_matrix.shape[:-2] != batch_shape + time_shape:
            transition_matrix = transition_matrix.expand(batch_shape + time_shape + (hidden_dim, hidden_dim))
        if transition_dist.batch_shape != batch_shape + time_shape:
            transition_dist = transition_dist.expand(batch_shape + time_shape)
        if observation_matrix.shape[:-2] != batch_shape + time_shape:
            observation_matrix = observation_matrix.expand(batch_shape + time_shape + (hidden_dim, obs_dim))
        if observation_dist.batch_shape != batch_shape + time_shape:
            observation_dist = observation_dist.expand(batch_shape + time_shape)

        # the observation transforms
        transforms = []
        while True:
            if isinstance(observation_dist, torch.distributions.Independent):
                observation_dist = observation_dist.base_dist
            elif isinstance(observation_dist, torch.distributions.TransformedDistribution):
                transforms = list(observation_dist.transforms) + transforms
                observation_dist = observation_dist.base_dist
            else:
                break
        if not observation_dist.event_shape:
            from . import Independent
            observation_dist = Independent(observation_dist, 1)

        self.hidden_dim, self.obs_dim = hidden_dim, obs_dim
        self.initial_dist = initial_dist
        self.transition_matrix = transition_matrix
        self.transition_dist = transition_dist
        self.observation_matrix = observation_matrix
        self.observation_dist = observation_dist
        self.transforms = transforms

    def _init_duration(self, duration, event_shape):
        """The reference's duration rule (hmm.py:200-215) -> the event shape, its time axis named by ``duration``."""
        if duration is None:
            if event_shape[0] != 1:
                duration = event_shape[0]
        elif duration != event_shape[0]:
            if event_shape[0] != 1:
                raise ValueError("duration, event_shape mismatch: {} vs {}".format(duration, event_shape))
            event_shape = (duration,) + tuple(event_shape[1:])
        self.duration = duration
        return torch.Size(event_shape)

    @constraints.dependent_property(event_dim=2)
    def support(self):
        return constraints.independent(self.observation_dist.support, 1)

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(LinearHMM, _instance)
        batch_shape = torch.Size(batch_shape)
        time_shape = self.transition_dist.batch_shape[-1:]
        h, o = self.hidden_dim, self.obs_dim
        new.hidden_dim, new.obs_dim, new.duration = h, o, self.duration
        new.initial_dist = self.initial_dist.expand(batch_shape)
        new.transition_matrix = self.transition_matrix.expand(batch_shape + time_shape + (h, h))
        new.transition_dist = self.transition_dist.expand(batch_shape + time_shape)
        new.observation_matrix = self.observation_matrix.expand(batch_shape + time_shape + (h, o))
        new.observation_dist = self.observation_dist.expand(batch_shape + time_shape)
        new.transforms = self.transforms
        super(LinearHMM, new).__init__(batch_shape, self.event_shape, validate_args=False)
        new._validate_args = self.__dict__.get("_validate_args")
        return new

    def log_prob(self, value):
        raise NotImplementedError("LinearHMM.log_prob() is not implemented")

    def rsample(self, sample_shape=torch.Size(), *, noise=None):
        """Sample paths of the observations, ``sample_shape + batch_shape + (duration, obs_dim)`` (reference:
        hmm.py:1122-1138); needs ``duration``.

            z_0 = init,   z_t = z_{t-1} F_t + e_t,   x_t = transforms(z_t H_t + n_t)

        ``noise``: the triple ``(init, e, n)`` of DRAWS of the three component distributions (location and scale
        applied, not standard normals) of shapes ``sample_shape + batch_shape`` + ``(hidden_dim,)``,
        ``(duration, hidden_dim)`` and ``(duration, obs_dim)``.  (The keyword is this package's, as for
        ``GaussianHMM.rsample``.)  Not given, it is the three components' own ``rsample(sample_shape)`` in the
        reference's order: initial, transition expanded to the duration, then observation.

        Device tensors of one dtype, float32 or float64, with hidden and obs dimension up to 16 and nothing requiring
        a gradient under grad mode take the ONE launch of csrc/linear_hmm.hip and the result is DETACHED.  Everything
        else -- grad mode with a matrix or the noise (hence a component's parameter) requiring a gradient, CPU
        tensors, larger dimensions, other or mixed dtypes, ``hmm.FUSED_LINEAR_HMM = False`` -- is the loop in torch
        ops: reparameterised in the matrices and, through the components' ``rsample``, in their parameters.  The
        transforms are applied by torch after either route."""
        if self.duration is None:
            raise ValueError("LinearHMM.rsample needs a duration (time-homogeneous parameters do not tell it)")
        T, h, o = self.duration, self.hidden_dim, self.obs_dim
        sample_shape = torch.Size(sample_shape)
        shape = sample_shape + self.batch_shape
        shapes = (shape + (h,), shape + (T, h), shape + (T, o))
        if noise is None:
            init = self.initial_dist.rsample(sample_shape)
            e = self.transition_dist.expand(self.batch_shape + (T,)).rsample(sample_shape)
            n = self.observation_dist.expand(self.batch_shape + (T,)).rsample(sample_shape)
            noise = (init, e, n)
        else:
            noise = tuple(noise)
            if len(noise) != 3 or any(e.shape != s for e, s in zip(noise, shapes)):
                raise ValueError("expected noise as a triple of shapes {}, {} and {}, got {}".format(
                    *(tuple(s) for s in shapes), [tuple(e.shape) for e in noise]))
        F, H = self.transition_matrix, self.observation_matrix
        tensors = (F, H) + noise
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
        from .. import kernels
        if (not needs_grad and FUSED_LINEAR_HMM and F.dtype in (torch.float32, torch.float64)
                and all(kernels.on_device(t) and t.dtype == F.dtype for t in tensors)
                and h <= kernels.GAUSSIAN_HMM_MAX_HIDDEN and o <= kernels.GAUSSIAN_HMM_MAX_OBS
                and self.batch_shape.numel() > 0):
            nb, B = len(self.batch_shape), self.batch_shape.numel()
            mats = [_kernel_matrix(m.detach(), nb) for m in (F, H)]
            draws = [t.detach().reshape((-1, B) + tuple(s[len(shape):])).contiguous() for t, s in zip(noise, shapes)]
            x, _ = kernels.linear_hmm_draw(*mats, T, *draws)
            x = x.reshape(shapes[2])
        else:
            z, (e, n) = noise[0], noise[1:]
            xs = []
            for t in range(T):
                z = (z.unsqueeze(-2) @ _step(F, t, 2)).squeeze(-2) + e[..., t, :]
                xs.append((z.unsqueeze(-2) @ _step(H, t, 2)).squeeze(-2) + n[..., t, :])
            x = torch.stack(xs, dim=-2)
        for t in self.transforms:
            x = t(x)
        return x


class IndependentHMM(TorchDistribution):
    """A batch of independent univariate HMMs seen as one multivariate distribution (reference:
    pyro/distributions/hmm.py:1141-1198): ``base_dist`` with batch shape ``shape + (obs_dim,)`` and event shape
    ``(duration, 1)`` becomes a distribution with batch shape ``shape`` and event shape ``(duration, obs_dim)``."""
    arg_constraints = {}

    def __init__(self, base_dist):
        if not base_dist.batch_shape or len(base_dist.event_shape) != 2 or base_dist.event_shape[-1] != 1:
            raise ValueError("expected a base HMM with at least one batch dim and event shape (duration, 1), got "
                             "batch shape {} and event shape {}".format(tuple(base_dist.batch_shape),
                                                                        tuple(base_dist.event_shape)))
        batch_shape = base_dist.batch_shape[:-1]
        event_shape = base_dist.event_shape[:-1] + base_dist.batch_shape[-1:]
        super().__init__(batch_shape, event_shape)
        self.base_dist = base_dist

    @constraints.dependent_property(event_dim=2)
    def support(self):
        return self.base_dist.support

    @property
    def has_rsample(self):
        return self.base_dist.has_rsample

    @property
    def duration(self):
        return self.base_dist.duration

    def expand(self, batch_shape, _instance=None):
        batch_shape = torch.Size(batch_shape)
        new = self._get_checked_instance(IndependentHMM, _instance)
        new.base_dist = self.base_dist.expand(batch_shape + self.base_dist.batch_shape[-1:])
        super(IndependentHMM, new).__init__(batch_shape, self.event_shape, validate_args=False)
        new._validate_args = self.__dict__.get("_validate_args")
        return new

    def _validate_sample(self, value):
        pass        # the base distribution checks what it is given

    def rsample(self, sample_shape=torch.Size()):
        base_value = self.base_dist.rsample(sample_shape)
        return base_value.squeeze(-1).transpose(-1, -2)

    def log_prob(self, value):
        base_value = value.transpose(-1, -2).unsqueeze(-1)
        return self.base_dist.log_prob(base_value).sum(-1)
