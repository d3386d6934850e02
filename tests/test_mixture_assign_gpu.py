"""csrc/mixture_assign.hip on the device against float64 torch (tests/assign_cases.py): the most probable component
and the inverse-CDF draw of every row, over every lane layout, ragged row counts, weight layouts, families and dtypes;
edge rows, limits, reproducibility; and infer_discrete's fast route against its generic route on the same uniforms.

Rows the float64 reference cannot decide are left out: for MAP those whose top two scores lie closer than
margin * max(1, |m|), for a draw those where u c_{K-1} lies within margin * c_{K-1} of a c_k; margin 1e-10 in float64,
1e-4 in float32 (float32 log-densities of magnitude up to ~100 carry ~1e-5 absolute error).  At most 1 % (MAP) and
3 % (draw) of a case's rows may be left out; for the seeds below the reference alone stays under that."""
import ctypes

import pytest
import torch

from tests.assign_cases import (F32_MARGIN, F64_MARGIN, assign_scores, draw_reference, fitted_mixture, flat,
                                kernel_case, lay_out, map_reference, philox_uniforms)
from tests.event_mixture_cases import FAMILIES, dist_id

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x5EED1234ABCD, 977


def _margin(dtype):
    return F32_MARGIN if dtype == torch.float32 else F64_MARGIN


def _run(case, family, B, layout, dtype, gpu, mode, seed=SEED, offset=OFFSET):
    """-> (z from the kernel [B, N], float64 scores of the SAME rounded inputs [B, N, K])"""
    from pyro_amd import kernels

    x = case["x"].to(gpu, dtype)
    a = lay_out(case["a"].to(gpu, dtype), B, layout)
    p0 = case["p0"].to(gpu, dtype)
    p1 = None if case["p1"] is None else case["p1"].to(gpu, dtype)
    K = a.shape[-1]
    if x.dim() == 2:
        z = kernels.mixture_assign_diag_normal(x, a, p0, p1, mode=mode, seed=seed, offset=offset)
    else:
        f0, s0, bs0 = flat(p0, B, K)
        f1, s1, bs1 = flat(p1, B, K)
        z = kernels.mixture_assign(dist_id(family), x, a, f0, s0, f1, s1, bs0, bs1, mode=mode, seed=seed,
                                   offset=offset)
    assert z.dtype == torch.int64 and z.shape == (B, x.shape[0]) and z.is_contiguous()
    t = assign_scores(family, x, a, p0.expand((B,) + tuple(p0.shape[1:])),
                      None if p1 is None else p1.expand((B,) + tuple(p1.shape[1:])))
    return z, t


def _check(case, family, B, layout, dtype, gpu):
    N = case["x"].shape[0]
    z, t = _run(case, family, B, layout, dtype, gpu, 0)
    want, keep = map_reference(t, _margin(dtype))
    left = 1.0 - keep.double().mean().item()
    print("MAP  %s N=%d left out %.4f" % (family, N, left))
    assert left <= 0.01
    assert bool((z == want)[keep].all()), (z[keep & (z != want)][:8], want[keep & (z != want)][:8])
    z, t = _run(case, family, B, layout, dtype, gpu, 1)
    u = philox_uniforms(B, N, dtype, SEED, OFFSET, gpu)
    want, keep = draw_reference(t, u, _margin(dtype))
    left = 1.0 - keep.double().mean().item()
    print("draw %s N=%d left out %.4f" % (family, N, left))
    assert left <= 0.03
    assert bool((z == want)[keep].all()), (z[keep & (z != want)][:8], want[keep & (z != want)][:8])
    assert int(z.min()) >= 0 and int(z.max()) < t.shape[-1]


LAYOUTS = ("shared", "rows", "sets", "sliced")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 16, 33, 64])
def test_every_lane_layout_and_ragged_row_count(gpu, K, dtype):
    """KP = 1 .. 64 (one lane per row .. one row per wave), N ragged against the rows per wave, N = 4099 and 20 011:
    the four-deep loop runs twice per wave and ends part-way (4 waves of 64 / KP rows per workgroup, eight iterations
    per wave aimed at: 5.3 to 8 iterations at these sizes), B = 1 and 3, the weight layouts in turn."""
    i = 0
    for N in (1, 63, 4099, 20_011):
        for B in (1, 3):
            layout = LAYOUTS[i % 4]
            i += 1
            _check(kernel_case("Normal", N, K, B, layout=layout, seed=200 + K), "Normal", B, layout, dtype, gpu)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_weight_layouts(gpu, layout, dtype):
    _check(kernel_case("Normal", 4099, 5, 3, layout=layout, seed=7), "Normal", 3, layout, dtype, gpu)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("share", [None, "k", "b"])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_family_and_shared_parameters(gpu, family, share, dtype):
    _check(kernel_case(family, 4099, 5, 3, layout="rows", share=share, seed=11), family, 3, "rows", dtype, gpu)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D,K,B,layout,share", [(1, 3, 1, "shared", None), (3, 5, 3, "rows", "k"),
                                                (8, 33, 3, "sliced", "b"), (8, 16, 1, "sets", None)])
def test_diagonal_normal(gpu, D, K, B, layout, share, dtype):
    for N in (63, 4099):
        _check(kernel_case("Normal", N, K, B, D=D, layout=layout, share=share, seed=13), "Normal", B, layout, dtype,
               gpu)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_exact_tie_returns_the_lower_index(gpu, dtype):
    """two identical components (2 and 4 of 6), everywhere the best: MAP returns 2"""
    from pyro_amd import kernels

    N, K = 1000, 6
    x = torch.linspace(-1.0, 1.0, N, dtype=dtype, device=gpu)
    loc = torch.tensor([9.0, -9.0, 0.0, 7.0, 0.0, -7.0], dtype=dtype, device=gpu)
    scale = torch.ones(K, dtype=dtype, device=gpu)
    a = torch.zeros(1, K, dtype=dtype, device=gpu)
    z = kernels.mixture_assign(dist_id("Normal"), x, a, loc, 1, scale, 1)
    assert bool((z == 2).all())
    zd = kernels.mixture_assign_diag_normal(x[:, None].contiguous(), a, loc.reshape(1, K, 1), scale.reshape(1, K, 1))
    assert bool((zd == 2).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", [0, 1])
def test_edge_rows_and_memory_past_the_end(gpu, mode, dtype):
    """A row of all -inf weights and a row with a NaN observation give 0, their neighbours are what they are without
    them; a component switched off is never returned; nothing is written past z (z's memory is taken out of a larger
    buffer of sentinels through the C entry point)."""
    from pyro_amd import _lib, kernels

    N, K, B = 4099, 5, 3
    case = kernel_case("Normal", N, K, B, layout="rows", seed=17)
    clean, _ = _run(case, "Normal", B, "rows", dtype, gpu, mode)
    a = case["a"].clone()
    a[:, :, 3] = -float("inf")                     # component 3 switched off
    a[1, 77, :] = -float("inf")
    a[:, 4098, :] = -float("inf")
    x = case["x"].clone()
    x[100] = float("nan")
    edge = dict(case, a=a, x=x)
    z, t = _run(edge, "Normal", B, "rows", dtype, gpu, mode)
    assert int(z[1, 77]) == 0 and bool((z[:, 4098] == 0).all()) and bool((z[:, 100] == 0).all())
    assert not bool((z == 3).any())
    if mode == 0:
        want, keep = map_reference(t, _margin(dtype))
    else:
        want, keep = draw_reference(t, philox_uniforms(B, N, dtype, SEED, OFFSET, gpu), _margin(dtype))
    assert bool((z == want)[keep].all())
    same = clean != 3                               # rows that did not pick the switched-off component before
    same[:, [100, 4098]] = False
    same[1, 77] = False
    if mode == 0:
        assert bool((z == clean)[same].all())
    # through the C entry point into the middle of a buffer of sentinels
    pad = 1024
    buf = torch.full((pad + B * N + pad,), -7, dtype=torch.int64, device=gpu)
    xd, ad = x.to(gpu, dtype), a.to(gpu, dtype).contiguous()
    p0, p1 = case["p0"].to(gpu, dtype).reshape(-1), case["p1"].to(gpu, dtype).reshape(-1)
    rc = _lib.load().pa_mixture_assign(kernels._dtype(xd), dist_id("Normal"), kernels._ptr(xd), N, K, B,
                                       kernels._ptr(ad), 1, K, N * K, kernels._ptr(p0), 1, K, kernels._ptr(p1), 1, K,
                                       mode, SEED, OFFSET, None, ctypes.c_void_p(buf.data_ptr() + 8 * pad),
                                       kernels._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:pad] == -7).all()) and bool((buf[pad + B * N:] == -7).all())
    assert torch.equal(buf[pad:pad + B * N].reshape(B, N), z)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_draws_are_reproducible_and_follow_the_offset(gpu, dtype):
    case = kernel_case("Normal", 4099, 5, 3, layout="rows", seed=19)
    z1, _ = _run(case, "Normal", 3, "rows", dtype, gpu, 1)
    z2, _ = _run(case, "Normal", 3, "rows", dtype, gpu, 1)
    z3, _ = _run(case, "Normal", 3, "rows", dtype, gpu, 1, offset=OFFSET + 5000)
    assert torch.equal(z1, z2) and not torch.equal(z1, z3)
    cased = kernel_case("Normal", 4099, 5, 3, D=3, layout="shared", seed=19)
    d1, _ = _run(cased, "Normal", 3, "shared", dtype, gpu, 1)
    d2, _ = _run(cased, "Normal", 3, "shared", dtype, gpu, 1)
    assert torch.equal(d1, d2)


def test_limits_are_refused_before_any_launch(gpu):
    from pyro_amd import _lib

    lib = _lib.load()
    F32, U = _lib.PA_F32, _lib.PA_ERR_UNSUPPORTED
    normal = dist_id("Normal")
    assert lib.pa_mixture_assign(F32, normal, None, 10, 65, 1, None, 1, 65, 0, None, 1, 0, None, 1, 0, 0, 0, 0, None,
                                 None, None) == U
    assert lib.pa_mixture_assign(F32, normal, None, 10, 4, 65536, None, 1, 4, 0, None, 1, 0, None, 1, 0, 0, 0, 0, None,
                                 None, None) == U
    assert lib.pa_mixture_assign_diag_normal(F32, None, 10, 9, 4, 1, None, 1, 4, 0, None, 9, 1, 0, None, 9, 1, 0, 0,
                                             0, 0, None, None, None) == U
    assert lib.pa_mixture_assign_diag_normal(F32, None, 10, 3, 65, 1, None, 1, 65, 0, None, 3, 1, 0, None, 3, 1, 0,
                                             0, 0, 0, None, None, None) == U
    assert lib.pa_mixture_assign_diag_normal(F32, None, 10, 3, 4, 65536, None, 1, 4, 0, None, 3, 1, 0, None, 3, 1, 0,
                                             0, 0, 0, None, None, None) == U


# ---- through infer_discrete ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "gate", "sets"])
@pytest.mark.parametrize("temperature", [0, 1])
def test_infer_discrete_fast_route_equals_the_generic_route(gpu, monkeypatch, temperature, form):
    """float64, so that the two routes' arithmetic differs by ~1e-16 relative and no row of 4099 is undecided"""
    import pyro_amd as pyro
    import pyro_amd.ops.contract as c
    from pyro_amd import kernels
    from pyro_amd.infer import infer_discrete

    N, K, B = 4099, 5, 3
    model = fitted_mixture(form, gpu, torch.float64, N, K, B)
    calls = []
    for name in ("mixture_assign", "mixture_assign_diag_normal"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, (lambda real: lambda *a, **k: (calls.append(1), real(*a, **k))[1])(real))
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(c, "FUSED_MIXTURE", fused)
        pyro.set_rng_seed(5)
        out[fused] = infer_discrete(model, first_available_dim=-3, temperature=temperature)()
        assert len(calls) == 1, (fused, calls)
    assert out[True].shape == ((B, N) if form == "sets" else (N,)) and out[True].dtype == torch.int64
    assert torch.equal(out[True], out[False])
    assert len(torch.unique(out[True])) > 1


def test_fast_route_allocates_nothing_of_size_k_n(gpu):
    """N = 200 000, K = 16, float32: the peak over one fast-route call stays below one [K, N] frame (12.8 MB) on top of
    what was allocated before the call -- it allocates z (1.6 MB) and [K]-sized pieces."""
    import pyro_amd as pyro
    from pyro_amd.infer import infer_discrete

    N, K = 200_000, 16
    model = fitted_mixture("plain", gpu, torch.float32, N, K)
    for temperature in (0, 1):
        pyro.set_rng_seed(1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        z = infer_discrete(model, first_available_dim=-2, temperature=temperature)()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
        print("temperature %d: %.2f MB above the inputs" % (temperature, extra / 1e6))
        assert extra < K * N * 4, extra
        assert z.shape == (N,)
