"""csrc/logchain_decode.hip on the device against the float64 torch restatement of tests/chain_decode_cases.py: the
most probable path and the posterior draw of a chain, over every launch path (the register layouts for K <= 16 and
K <= 32 with their prefetch depths 8 / 4 / 2, the lane-per-state kernel up to 64), the three pairwise layouts, both
dtypes; edge sequences, limits, reproducibility; and infer_discrete's chain route against its generic route.

The restatement is teacher-forced with the kernel's own z_{t-1}; steps it cannot decide are left out: for the most
probable path those whose top two scores lie closer than margin * max(1, |m|), for a draw those where u c_{K-1} lies
within margin * c_{K-1} of a c_k.  margin: 1e-10 in float64.  In float32 the backward messages gather error over T:
measured here as the worst |m_f32 - m_f64| / max(1, |m_f64|) of the restatement run in float32 on the CPU over the
longest inputs of every K and layout of this file: 5.0e-7; four times that stays below the 1e-4 of the assignment
tests, which is therefore the margin (test_f32_margin_covers_the_message_error measures and checks it).  At most 1 %
(path) and 3 % (draw) of a case's steps may be left out; the seed of a case is the first for which the restatement
alone, decoding on the CPU, stays under that."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import assign_cases as ac
from tests import chain_decode_cases as cc

SEED, OFFSET = 0x5EED1234ABCD, 977
KS = (1, 2, 3, 16, 17, 32, 33, 64)
BS = (1, 3, 65)
CAP = {0: 0.01, 1: 0.03}
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lengths(K):
    """T = 1, 2, 3 and D, D + 1, 2 D + 1 for the prefetch depths D of the register layouts (8 for K <= 16; 4 in
    float32 and 2 in float64 for K <= 32); 40 for the lane-per-state kernel"""
    return (1, 2, 3, 8, 9, 17) if K <= 16 else (1, 2, 3, 4, 5, 9) if K <= 32 else (1, 2, 3, 40)


def _margin(dtype):
    return ac.F32_MARGIN if dtype == torch.float32 else ac.F64_MARGIN


def _blocks(B, dtype):
    per = 4 if dtype == torch.float32 else 2
    return (B + per - 1) // per


@functools.lru_cache(maxsize=None)
def _case(B, T, K, layout, dtype, mode):
    """(U, P, seed) on the CPU in ``dtype``: the first seed for which the restatement's own decoding leaves out no more
    than the cap"""
    for seed in range(20):
        U, P = cc.chain_case(B, T, K, layout, seed, dtype)
        z, _ = cc.decode_standin()(U, P, mode, SEED, OFFSET, None, _blocks(B, dtype))
        keep = cc.decode_reference(U, P, mode, z, _margin(dtype), SEED, OFFSET, _blocks(B, dtype))[1]
        if 1.0 - keep.double().mean().item() <= CAP[mode]:
            return U, P, seed
    raise AssertionError("no seed under the cap")


def _decode(U, P, mode, gpu, seed=SEED, offset=OFFSET, offset_dev=None):
    from pyro_amd import kernels

    B, T, K = U.shape
    z, norm = kernels.logchain_decode(U.to(gpu), None if P is None else P.to(gpu), mode=mode, seed=seed, offset=offset,
                                      offset_dev=offset_dev, step_blocks=_blocks(B, U.dtype))
    assert z.dtype == torch.int64 and z.shape == (B, T) and z.is_contiguous()
    assert norm.dtype == U.dtype and norm.shape == (B,)
    return z.cpu(), norm.cpu()


def _check(U, P, mode, gpu, what):
    B, T, K = U.shape
    dtype = U.dtype
    z, norm = _decode(U, P, mode, gpu)
    assert bool(((z >= 0) & (z < K)).all())
    want, keep, ref_norm = cc.decode_reference(U, P, mode, z, _margin(dtype), SEED, OFFSET, _blocks(B, dtype))
    left = 1.0 - keep.double().mean().item()
    print("%s mode %d left out %.4f" % (what, mode, left))
    assert left <= CAP[mode], what
    bad = keep & (z != want)
    assert not bool(bad.any()), (what, bad.nonzero()[:8], z[bad][:8], want[bad][:8])
    tol = 64 * torch.finfo(dtype).eps * (1 + T)
    assert torch.allclose(norm.double(), ref_norm, rtol=tol, atol=tol), (what, norm, ref_norm)
    if mode == 0 and K ** T <= 1e5 and B <= 3:
        got = cc.path_scores(U, None if P is None else cc.full_pairwise(P, B, T), z)
        for b in range(B):
            best = cc.best_path_score(U, P, b)
            assert abs(float(got[b] - best)) <= 2 * _margin(dtype) * max(1.0, abs(float(best))), (what, b)
    return z, norm


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kernel_against_the_restatement(gpu, dtype, mode, K):
    from pyro_amd import kernels

    for T in _lengths(K):
        for layout in cc.LAYOUTS if T > 1 else ("shared",):
            for B in BS:
                U, P, seed = _case(B, T, K, layout, dtype, mode)
                what = "K=%d T=%d B=%d %s seed %d %s" % (K, T, B, layout, seed, dtype)
                _, norm = _check(U, P, mode, gpu, what)
                if mode == 1 and T > 1:
                    log_z = kernels.logchain_fwd_bwd(U.to(gpu), P.to(gpu))[0].cpu()
                    tol = 64 * torch.finfo(dtype).eps * (1 + T)
                    assert torch.allclose(norm, log_z, rtol=tol, atol=tol), what


def test_f32_margin_covers_the_message_error():
    """(on the CPU) four times the float32 restatement's worst message error stays below F32_MARGIN"""
    worst = 0.0
    for mode in (0, 1):
        for K in KS:
            for layout in cc.LAYOUTS:
                U, P = cc.chain_case(65, _lengths(K)[-1], K, layout, 0, torch.float32)
                worst = max(worst, cc.message_error_f32(U, P, mode))
    print("worst float32 message error %.3g" % worst)
    assert 4 * worst <= ac.F32_MARGIN


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K,T", [(5, 12), (24, 9), (40, 11)])
def test_left_to_right_chains(gpu, mode, K, T):
    """-inf transitions: no way back to a lower state"""
    for dtype in (torch.float32, torch.float64):
        for seed in range(20):
            U, P = cc.chain_case(7, T, K, "per_step", seed, dtype, left_to_right=True)
            zc, _ = cc.decode_standin()(U, P, mode, SEED, OFFSET, None, _blocks(7, dtype))
            keep = cc.decode_reference(U, P, mode, zc, _margin(dtype), SEED, OFFSET, _blocks(7, dtype))[1]
            if 1.0 - keep.double().mean().item() <= CAP[mode]:
                break
        z, _ = _check(U, P, mode, gpu, "left-to-right K=%d %s" % (K, dtype))
        assert bool((z[:, 1:] >= z[:, :-1]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K,T", [(3, 9), (20, 6), (64, 5)])
def test_dead_and_nan_sequences(gpu, mode, K, T):
    dtype = torch.float64
    U, P = cc.chain_case(6, T, K, "per_batch", 1, dtype)
    z0, n0 = _decode(U, P, mode, gpu)
    V = U.clone()
    V[2] = -float("inf")                                  # a sequence without a finite score
    V[4, T // 2, K // 2] = float("nan")                   # a NaN in the middle of another
    z, norm = _decode(V, P, mode, gpu)
    assert bool((z[2] == 0).all()) and float(norm[2]) == -float("inf")
    assert int(z[4, T // 2]) == 0 and bool((z[4, :T // 2] == 0).all()) and bool(torch.isnan(norm[4]))
    others = [0, 1, 3, 5]
    assert torch.equal(z[others], z0[others]) and torch.equal(norm[others], n0[others])
    # after the NaN the chain goes on from state 0: the restatement, teacher-forced, agrees
    want, keep, _ = cc.decode_reference(V, P, mode, z, ac.F64_MARGIN, SEED, OFFSET, _blocks(6, dtype))
    assert bool((z == want)[keep].all())


@pytest.mark.gpu
def test_limits(gpu):
    from pyro_amd import _lib, kernels

    z, norm = kernels.logchain_decode(torch.zeros((0, 4, 3), device=gpu), torch.zeros((3, 3), device=gpu))
    assert z.shape == (0, 4) and norm.shape == (0,)
    with pytest.raises(_lib.Unsupported):
        kernels.logchain_decode(torch.zeros((2, 3, 65), device=gpu), torch.zeros((65, 65), device=gpu))
    z, norm = kernels.logchain_decode(torch.zeros((2, 1, 5), device=gpu), None)      # T = 1 needs no pairwise
    assert bool((z == 0).all()) and torch.equal(norm.cpu(), torch.zeros(2))
    lib = _lib.load()
    u = torch.zeros((2, 3, 5), device=gpu)
    zz = torch.zeros((2, 3), dtype=torch.int64, device=gpu)
    nn = torch.zeros((2,), device=gpu)
    ws = torch.zeros((lib.pa_logchain_decode_workspace(_lib.PA_F32, 2, 3, 5),), dtype=torch.uint8, device=gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                  # noqa: E731
    rc = lib.pa_logchain_decode(_lib.PA_F32, p(u), None, 0, 0, 2, 3, 5, 0, 0, 0, None, 0, p(zz), p(nn), p(ws),
                                ws.numel(), None)
    assert rc == _lib.PA_ERR_INVALID and b"NULL pairwise" in lib.pa_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [7, 20, 50])
def test_draws_are_reproducible_and_follow_the_offset(gpu, K):
    for dtype in (torch.float32, torch.float64):
        U, P = cc.chain_case(33, 12, K, "per_step", 2, dtype)
        z, _ = _decode(U, P, 1, gpu)
        again, _ = _decode(U, P, 1, gpu)
        assert torch.equal(z, again)
        other, _ = _decode(U, P, 1, gpu, offset=OFFSET + 5000)
        assert not torch.equal(z, other)
        base = torch.tensor([OFFSET - 77, 0], dtype=torch.int64, device=gpu)
        shifted, _ = _decode(U, P, 1, gpu, offset=77, offset_dev=base)
        assert torch.equal(z, shifted)


# ---- infer_discrete on the device --------------------------------------------------------------------------------
def _infer(model, temperature, fused, seed, first_available_dim):
    import pyro_amd.ops.contract as c
    from pyro_amd.infer import infer_discrete

    keep, c.FUSED_CHAIN = c.FUSED_CHAIN, fused
    try:
        torch.manual_seed(seed)
        xs = infer_discrete(model, first_available_dim=first_available_dim, temperature=temperature)()
    finally:
        c.FUSED_CHAIN = keep
    return torch.stack([x.reshape(-1) for x in xs], -1).cpu()           # [B, T]


def _hmm(gpu, plated):
    T = ac.hmm_tensors(5, 3, seed=0, device=gpu)
    if not plated:
        return T, ac.make_hmm(T), T["data"][None], -1
    T["data"] = torch.randint(0, 4, (3, 5), generator=torch.Generator().manual_seed(5)).to(gpu)
    return T, cc.make_plated_hmm(T, 3), T["data"], -2


def _decided_seed(T, data):
    """the first seed at which the restatement, decoding on the CPU, decides every step by more than the margin"""
    from pyro_amd import rng

    U, P = cc.hmm_chain_potentials({k: v.cpu() for k, v in T.items()}, data.cpu())
    B = U.shape[0]
    for seed in range(20):
        torch.manual_seed(seed)
        ps = rng.current_seed()
        z, _ = cc.decode_standin()(U, P, 1, ps, 0, None, _blocks(B, U.dtype))
        if bool(cc.decode_reference(U, P, 1, z, 1e-6, ps, 0, _blocks(B, U.dtype))[1].all()):
            return seed
    raise AssertionError("no decided seed")


@pytest.mark.gpu
@pytest.mark.parametrize("plated", [False, True])
def test_infer_discrete_draws_equal_the_generic_routes(gpu, plated):
    from pyro_amd import kernels

    T, model, data, fad = _hmm(gpu, plated)
    seed = _decided_seed(T, data)
    calls = []
    real = kernels.logchain_decode
    kernels.logchain_decode = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        fast = _infer(model, 1, True, seed, fad)
        assert len(calls) == 1
        generic = _infer(model, 1, False, seed, fad)
        assert len(calls) == 1
    finally:
        kernels.logchain_decode = real
    assert fast.shape == (data.shape[0], 5) and torch.equal(fast, generic)


@pytest.mark.gpu
@pytest.mark.parametrize("plated", [False, True])
def test_infer_discrete_path_is_a_viterbi_path(gpu, plated):
    T, model, data, fad = _hmm(gpu, plated)
    xs = _infer(model, 0, True, 0, fad)
    cfg = ac.all_configs([3] * 5)
    host = {k: v.cpu() for k, v in T.items()}
    for b in range(data.shape[0]):
        host["data"] = data[b].cpu()
        best = ac.hmm_log_joint(host, cfg).max()
        assert abs(float(ac.hmm_log_joint(host, xs[b]) - best)) <= 1e-12 * abs(float(best))


@pytest.mark.gpu
def test_infer_discrete_path_has_the_references_joint_score(gpu):
    g = np.load(os.path.join(GOLDEN_DIR, "infer_discrete.npz"))
    host = {k: torch.as_tensor(g["hmm/" + k]) for k in ("init", "tp", "ep", "data")}
    T = {k: v.to(gpu) for k, v in host.items()}
    xs = _infer(ac.make_hmm(T), 0, True, 0, -1)[0]
    want = torch.as_tensor(g["hmm/xs"])
    assert abs(float(ac.hmm_log_joint(host, xs) - ac.hmm_log_joint(host, want))) <= 1e-9


@pytest.mark.gpu
def test_a_trace_of_the_decoded_model_has_the_kernels_values(gpu):
    from pyro_amd import kernels, poutine
    from pyro_amd.infer import infer_discrete

    T, model, data, fad = _hmm(gpu, False)
    U, P = cc.hmm_chain_potentials(T, data)
    z, _ = kernels.logchain_decode(U, P, mode=0)
    tr = poutine.trace(infer_discrete(model, first_available_dim=fad, temperature=0)).get_trace()
    for t in range(5):
        assert int(tr.nodes["x_{}".format(t)]["value"]) == int(z[0, t])
