"""What the layer-kernel edge tests rest on and a CPU can hold: the three-piece bf16 split as torch's own
round-to-nearest conversion does it (the written-down meaning of "exact" that the GPU cases are compared with), the
bound on the dropped piece products, the float64 oracle of oracle/lda.py on the small grids, and the constants of
the tolerance rule."""
import math

import numpy as np
import torch

from tests import layer_edge_cases as L


def _exact(x):
    p1, p2, p3 = L.split3(x)
    s = p1.double() + p2.double() + p3.double()
    return torch.isfinite(s) & (s == x.double())


def test_split_is_exact_for_exponents_minus_110_to_126():
    g = torch.Generator().manual_seed(0)
    m = (1.0 + torch.rand((4096,), generator=g, dtype=torch.float64))
    for e in range(-110, 127):
        x = (m * 2.0 ** e).float()
        x = torch.cat([x, -x])
        assert bool(_exact(x).all()), e
    # the neighbours of every power of two
    for e in range(-110, 127):
        p = torch.tensor([2.0 ** e], dtype=torch.float32)
        lower = torch.nextafter(p, torch.tensor([0.0])) if e > -110 else p      # (exponent e - 1)
        nb = torch.stack([lower, p, torch.nextafter(p, torch.tensor([math.inf]))])
        assert bool(_exact(torch.cat([nb, -nb]).reshape(-1)).all()), e
    # and not outside: below 2^-110 the third piece falls under bf16's smallest denormal (2^-133) ...
    x = (m * 2.0 ** -118).float()
    assert not bool(_exact(x).all())
    err = (sum(p.double() for p in L.split3(x)) - x.double()).abs() / x.double().abs()
    assert float(err.max()) <= 2.0 ** -16
    # ... and from 0x7f7f8000 (3.39618e38, half way between bf16's largest finite value and 2^128) on the first piece
    # rounds to inf, the second is x - inf = -inf and the third inf - inf = NaN
    edge = torch.tensor([0x7f7f8000], dtype=torch.int32).view(torch.float32)
    big = torch.cat([edge, torch.tensor([3.4028234e38])])
    p1, p2, p3 = L.split3(big)
    assert bool((p1 == math.inf).all()) and bool((p2 == -math.inf).all()) and bool(torch.isnan(p3).all())
    assert bool(_exact(torch.nextafter(edge, torch.tensor([0.0]))).all())


def test_split_of_inf_is_nan_in_the_second_piece():
    for v in (math.inf, -math.inf):
        p1, p2, p3 = L.split3(torch.tensor([v]))
        assert float(p1) == v and math.isnan(float(p2)) and math.isnan(float(p3))
    assert all(math.isnan(float(p)) for p in L.split3(torch.tensor([math.nan])))


def test_dropped_piece_products_cost_less_than_one_unit():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn((200_000,), generator=g), torch.randn((200_000,), generator=g)
    (a1, a2, a3), (b1, b2, b3) = [[p.double() for p in L.split3(t)] for t in (a, b)]
    kept = a3 * b1 + a2 * b2 + a1 * b3 + a2 * b1 + a1 * b2 + a1 * b1
    exact = a.double() * b.double()
    assert float(((kept - exact).abs() / exact.abs()).max()) < L.U


def test_the_rule_can_see_a_lost_piece():
    assert L.c_rule(128) < 32 and L.c_rule(1) >= 1
    assert L.c_rule(100_000) == (1 + 4 * L.T_LONG * math.sqrt(100_000) / 30)
    # a third piece lost in one operand moves a product by up to 2^-16: on one term, 256 units
    x = torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -17 + 2.0 ** -23])
    p1, p2, p3 = L.split3(x)
    assert float(p3) != 0 and abs(float(p3)) / float(x) > 32 * L.U


def test_float64_oracle_on_the_small_grids():
    """oracle/lda.py's restatements (what the existing kernel tests trust) against a plain float64 @ on the shapes
    of the grids; the reference is finite and inside the rule with c = 0 (it IS the reference) on every case."""
    from oracle import lda as o_lda
    dev = torch.device("cpu")
    for R, C in L.LINEAR_RC:
        for B in (1, 33, 129):
            g = L.gen(B + R + C, dev)
            x, W, b, go = (L.randn(s, g, dev).numpy() for s in ((B, R), (C, R), (C,), (B, C)))
            ref = x.astype(np.float64) @ W.astype(np.float64).T + b
            out = o_lda.tall_linear(x, W, b)
            assert np.isfinite(out).all() and np.array_equal(out, ref)
            dx, dW, db = o_lda.tall_linear_grads(x, W, go)
            go64 = go.astype(np.float64)
            assert np.array_equal(dx, go64 @ W.astype(np.float64))
            assert np.array_equal(dW, go64.T @ x.astype(np.float64)) and np.allclose(db, go64.sum(0), rtol=1e-15)
    for case in L.bow_cases(256):
        if case["B"] > 300:
            continue
        B, H, V, Wd = case["B"], case["H"], case["V"], case["Wd"]
        rng = np.random.default_rng(B + H)
        words = rng.integers(0, V, size=(Wd, B))
        W, b, d = rng.standard_normal((H, V)), rng.standard_normal(H), rng.standard_normal((B, H))
        counts = np.zeros((V, B))
        np.add.at(counts, (words, np.arange(B)[None, :].repeat(Wd, 0)), 1.0)
        assert np.allclose(o_lda.bow_linear(words, V, W, b), counts.T @ W.T + b, rtol=1e-14, atol=1e-12)
        dW, db = o_lda.bow_linear_grad(words, V, d)
        assert np.allclose(dW, d.T @ counts.T, rtol=1e-14, atol=1e-12) and np.allclose(db, d.sum(0))


def test_grids_cover_the_shapes_they_claim():
    cus = 256
    lin = L.linear_cases(cus)
    assert {c["B"] for c in lin} >= {1, 31, 32, 33, 127, 129, 4100, L.b16(cus) - 1, L.b16(cus), 100_000}
    assert {(c["R"], c["C"]) for c in lin} >= set(L.LINEAR_RC)
    assert {c["wkind"] for c in lin} == {"contig", "slice", "odd"} and {c["scale"] for c in lin} == {"none", "pow2", "cancel"}
    wg = L.wgrad_cases(cus)
    assert {c["R"] for c in wg} >= {1, 31, 32, 33, 64, 65, 96, 97, 128}
    assert {c["K"] for c in wg} >= {1, 32, 33, 64, 65, 96, 97, 128}
    assert {c["B"] for c in wg} >= {1, 15, 16, 17, 4097, 100_000, L.bw8(cus, 1), L.bw8(cus, 4) - 1}
    assert (L.b16(cus) + 31) // 32 == 4 * cus and (L.b16(cus) - 1 + 31) // 32 == 4 * cus - 1
    for nrt in (1, 2, 4):
        assert (L.bw8(cus, nrt) + 15) // 16 * nrt >= 24 * cus > (L.bw8(cus, nrt) - 1 + 15) // 16 * nrt


def test_launch_path_functions_without_a_device():
    """pa_tall_linear_path / pa_tall_wgrad_path launch nothing: their structure holds on any CU count."""
    from pyro_amd import _lib, kernels as k
    from pyro_amd.csrc.build import build_library
    build_library()
    cus = int(_lib.load().pa_device_cu_count())
    assert _lib.load().pa_tall_linear_path(10, 129, 4, 1, 129, 1, 1, 1) == -1
    assert _lib.load().pa_tall_wgrad_path(10, 4, 0) == -1
    for R, C, inst in ((16, 128, (1, 4)), (17, 32, (8, 1)), (17, 33, (7, 4)), (112, 128, (7, 4)), (113, 33, (8, 4)),
                       (113, 32, (8, 1)), (128, 128, (8, 4))):
        p = k.tall_linear_path(100, R, C, 1, R)
        assert (p["nks"], p["nct"]) == inst and p["stage"] == 0
    import os
    if os.environ.get("PA_TALL_WAVES") is None:
        assert k.tall_linear_path(L.b16(cus), 100, 100, 1, 100) == dict(nks=7, nct=4, nw=16, stage=1, wvec=0)
        assert k.tall_linear_path(L.b16(cus) - 1, 100, 100, 1, 100)["nw"] == 4
        assert k.tall_linear_path(L.b16(cus), 128, 128, 1, 128) == dict(nks=8, nct=4, nw=16, stage=0, wvec=1)
        assert k.tall_linear_path(L.b16(cus), 128, 128, 128, 1) == dict(nks=8, nct=4, nw=16, stage=0, wvec=0)
        assert k.tall_linear_path(1 << 22, 128, 4, 1, 128)["nw"] == 4
        assert k.tall_linear_path((1 << 22) - 1, 128, 4, 1, 128)["nw"] == 16
        assert k.tall_wgrad_path(L.bw8(cus, 4), 96, 100) == dict(nct=4, nw=8, nrt=4, jw=64)
        assert k.tall_wgrad_path(L.bw8(cus, 4) - 1, 96, 8) == dict(nct=1, nw=4, nrt=4, jw=16)
