"""Shared pieces of the chain decoding tests (kernels.logchain_decode, infer_discrete's chain route): a float64 torch
restatement of the kernel's two passes on the same rounded inputs cast up -- teacher-forced: given the kernel's own
z_{t-1} it says which z_t is wanted and where the choice is decided by more than a margin --, a stand-in for the kernel
built from it for the host tests, and the cases' inputs."""
import itertools

import torch

from tests.assign_cases import draw_reference, map_reference, philox_uniforms

LAYOUTS = ("shared", "per_step", "per_batch")


def chain_case(B, T, K, layout, seed, dtype=torch.float64, device="cpu", left_to_right=False):
    """randn-scaled log-probabilities: unary [B, T, K]; pairwise [K, K] ("shared"), [T-1, K, K] ("per_step") or
    [B, T-1, K, K] ("per_batch"), None for T = 1.  ``left_to_right``: -inf below the diagonal (no way back)."""
    g = torch.Generator().manual_seed(seed)
    U = torch.log_softmax(1.5 * torch.randn(B, T, K, generator=g, dtype=torch.float64), -1)
    if T == 1:
        return U.to(device, dtype), None
    lead = {"shared": (), "per_step": (T - 1,), "per_batch": (B, T - 1)}[layout]
    P = 1.5 * torch.randn(lead + (K, K), generator=g, dtype=torch.float64)
    if left_to_right:
        P = P.masked_fill(torch.ones(K, K).tril(-1).bool(), -float("inf"))
    P = torch.log_softmax(P, -1)
    return U.to(device, dtype).contiguous(), P.to(device, dtype).contiguous()


def full_pairwise(P, B, T):
    """pairwise in any of the three layouts -> the [B, T-1, K, K] view"""
    return P.expand((B, T - 1) + tuple(P.shape[-2:]))


def messages(U, P, mode):
    """m [B, T, K] in U's dtype: m_{T-1} = 0, m_t[i] = (+)_j (P_t[i, j] + u_{t+1}[j] + m_{t+1}[j])"""
    B, T, K = U.shape
    out = [None] * T
    out[T - 1] = torch.zeros_like(U[:, 0])
    Pf = None if T == 1 else full_pairwise(P, B, T)
    for t in range(T - 2, -1, -1):
        v = Pf[:, t] + (U[:, t + 1] + out[t + 1])[:, None, :]
        out[t] = v.max(-1).values if mode == 0 else torch.logsumexp(v, -1)
    return torch.stack(out, 1)


def step_scores(U, P, M, z):
    """s [B, T, K]: s_t[j] = (t ? P_{t-1}[z_{t-1}, j] : 0) + u_t[j] + m_t[j] with the given z [B, T] (teacher-forced)"""
    B, T, K = U.shape
    s = U + M
    if T > 1:
        Pf = full_pairwise(P, B, T)
        rows = torch.gather(Pf, 2, z[:, :-1, None, None].expand(B, T - 1, 1, K))[:, :, 0]
        s = torch.cat([s[:, :1], s[:, 1:] + rows], 1)
    return s


def chain_uniforms(B, T, dtype, seed, offset, step_blocks):
    """[B, T]: element b of the Philox uniform stream (seed, offset + t step_blocks), in ``dtype``"""
    return torch.stack([philox_uniforms(1, B, dtype, seed, offset + t * step_blocks)[0] for t in range(T)], 1)


def decode_reference(U, P, mode, z, margin, seed=0, offset=0, step_blocks=0):
    """The float64 restatement on the rounded inputs cast up, teacher-forced with the kernel's own z [B, T].
    -> (want [B, T], keep [B, T], log_norm [B])."""
    dtype = U.dtype
    U64 = U.detach().cpu().double()
    P64 = None if P is None else P.detach().cpu().double()
    z = z.detach().cpu()
    M = messages(U64, P64, mode)
    s = step_scores(U64, P64, M, z)
    if mode == 0:
        want, keep = map_reference(s, margin)
        return want, keep, s[:, 0].max(-1).values
    u = chain_uniforms(U.shape[0], U.shape[1], dtype, seed, offset, step_blocks)
    want, keep = draw_reference(s, u, margin)
    return want, keep, torch.logsumexp(s[:, 0], -1)


def decode_standin(calls=None):
    """A stand-in for kernels.logchain_decode built from the restatement (float64, one step after the other on its
    own z); every call is noted in ``calls`` as (B, T, K, mode, step_blocks)."""
    def logchain_decode(unary, pairwise, mode=0, seed=0, offset=0, offset_dev=None, step_blocks=0):
        B, T, K = unary.shape
        if calls is not None:
            calls.append((B, T, K, int(mode), int(step_blocks)))
        assert unary.is_contiguous() and (T == 1 or pairwise.is_contiguous()) and K <= 64 and offset_dev is None
        U64 = unary.detach().double()
        P64 = None if T == 1 else full_pairwise(pairwise.detach().double(), B, T)
        M = messages(U64, P64, mode)
        u = None if mode == 0 else chain_uniforms(B, T, unary.dtype, seed, offset, step_blocks)
        z = torch.zeros((B, T), dtype=torch.int64)
        norm = None
        for t in range(T):
            s = U64[:, t] + M[:, t]
            if t:
                s = s + P64[torch.arange(B), t - 1, z[:, t - 1]]
            if mode == 0:
                z[:, t] = map_reference(s[:, None], 0.0)[0][:, 0]
            else:
                z[:, t] = draw_reference(s[:, None], u[:, t:t + 1], 0.0)[0][:, 0]
            if t == 0:
                norm = s.max(-1).values if mode == 0 else torch.logsumexp(s, -1)
        return z, norm.to(unary.dtype)

    return logchain_decode


def path_scores(U, P, z):
    """the float64 joint score [B] of the paths z [B, T] (or [N, T] against B = 1 broadcast)"""
    U64 = U.detach().cpu().double()
    z = z.detach().cpu()
    B, T, K = U64.shape
    sc = torch.gather(U64.expand(z.shape[0], T, K), 2, z[:, :, None])[:, :, 0].sum(1)
    if T > 1:
        Pf = full_pairwise(P.detach().cpu().double(), B, T).expand(z.shape[0], T - 1, K, K)
        rows = torch.gather(Pf, 2, z[:, :-1, None, None].expand(-1, -1, 1, K))[:, :, 0]
        sc = sc + torch.gather(rows, 2, z[:, 1:, None])[:, :, 0].sum(1)
    return sc


def best_path_score(U, P, b):
    """the brute-force maximum over all K^T paths of sequence b, in float64"""
    B, T, K = U.shape
    cfg = torch.tensor(list(itertools.product(range(K), repeat=T)))
    Pb = None if P is None else full_pairwise(P, B, T)[b:b + 1]
    return path_scores(U[b:b + 1], Pb, cfg).max()


def message_error_f32(U, P, mode):
    """the worst |m_f32 - m_f64| / max(1, |m_f64|) of the backward messages run in float32 on float32-rounded inputs"""
    U32 = U.float()
    P32 = None if P is None else P.float()
    m32 = messages(U32, P32, mode).double()
    m64 = messages(U32.double(), None if P is None else P32.double(), mode)
    fin = torch.isfinite(m64)
    if not bool(fin.any()):
        return 0.0
    return float(((m32 - m64).abs() / m64.abs().clamp(min=1.0))[fin].max())


# ---- models ----------------------------------------------------------------------------------------------------------
def make_plated_hmm(T, B, backend=None):
    """tests.assign_cases.make_hmm for B sequences under a vectorised plate at dim -1: data [B, length]; returns the
    list of states, each [B]."""
    if backend is None:
        import pyro_amd as pyro
        import pyro_amd.distributions as dist
    else:
        pyro, dist = backend

    def model():
        xs = []
        with pyro.plate("sequences", B, dim=-1):
            x = None
            for i in pyro.markov(range(T["data"].shape[1])):
                probs = T["init"] if x is None else T["tp"][x]
                x = pyro.sample("x_{}".format(i), dist.Categorical(probs), infer={"enumerate": "parallel"})
                pyro.sample("y_{}".format(i), dist.Categorical(T["ep"][x]), obs=T["data"][:, i])
                xs.append(x)
        return xs

    return model


def hmm_chain_potentials(T, data):
    """(unary [B, length, S], pairwise [S, S]) of the HMM of tests.assign_cases.hmm_tensors for data [B, length]"""
    init, tp, ep = T["init"].log(), T["tp"].log(), T["ep"].log()
    U = ep.t()[data]                                    # [B, length, S]
    U = torch.cat([U[:, :1] + init, U[:, 1:]], 1)
    return U.contiguous(), tp.contiguous()
