"""The references of tests/enum_edge_cases.py against the project's numpy oracles, the launch-path
tables against the restated budget formulas, and the unscored-elements cap of every float32 grid entry
-- all on the CPU."""
import numpy as np
import pytest
import torch

from oracle import lda as o_lda
from oracle import logsumexp as o_lse
from tests import enum_edge_cases as ec
from tests import oracle_backend as ob


def _close(a, b, M):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        same = (np.isnan(a) == np.isnan(b)) & ((a == ec.INF) == (b == ec.INF)) & ((a == -ec.INF) == (b == -ec.INF))
        fin = np.isfinite(a) & np.isfinite(b)
        return bool((same & (~fin | (np.abs(a - b) <= 64 * ec.EPS64 * np.broadcast_to(M, a.shape)))).all())


def _small_chain_cases():
    out = []
    for f32 in (True, False):
        for K, T in ec.chain_grid(f32):
            if K ** T <= ec.BRUTE_PATHS:
                out += [(K, T, B, lay, f32, None) for B in ec.CHAIN_B for lay in ec.CHAIN_LAYOUTS if T > 1 or lay == "BTKK"]
        for K, T in ec.chain_pattern_shapes(f32):
            if K ** T <= ec.BRUTE_PATHS:
                out += [(K, T, 3, "BTKK", f32, p) for p in ec.CHAIN_PATTERNS]
    return sorted(set(out), key=str)


def test_chain_oracle_is_pinned_to_the_enumeration():
    """tests/oracle_backend.logchain_fwd_bwd (the reference of the shapes too large to enumerate) equals
    the sum over every path on every small case of the grid, the -inf / NaN / +inf patterns included."""
    n = 0
    for K, T, B, lay, f32, pat in _small_chain_cases():
        c = ec.chain_case(K, T, B, lay, f32, pat)
        assert c["brute"]
        with np.errstate(all="ignore"):
            got = [x.numpy() for x in ob.logchain_fwd_bwd(c["U"], c["P"])]
        lz = c["ref"][0]
        scored = np.isfinite(lz) | (lz == -ec.INF)              # gradients of a NaN / +inf chain: not scored
        assert _close(got[0], lz, c["M"]), (K, T, B, lay, pat)
        for g, r in zip(got[1:], c["ref"][1:]):
            assert _close(g[scored], r[scored], c["M"][scored].reshape((-1,) + (1,) * (r.ndim - 1))), \
                (K, T, B, lay, pat)
        n += 1
    assert n > 100


def test_chain_reference_properties():
    """What the patterns promise, on the reference itself: logZ = -inf and zero posteriors for the dead
    batch element, +inf for a +inf potential, NaN for a NaN, logZ shifted by 3e4 T under the constant
    shift with the posteriors unchanged, and P never symmetric."""
    for K, T in [(3, 4), (17, 2), (33, 2)]:
        clean = ec.chain_case(K, T, 3, "BTKK", False)
        assert not torch.equal(clean["P"], clean["P"].transpose(-1, -2))
        dead = ec.chain_case(K, T, 3, "BTKK", False, "dead_batch")
        assert dead["ref"][0][1] == -ec.INF and (dead["ref"][1][1] == 0).all() and (dead["ref"][2][1] == 0).all()
        assert np.array_equal(dead["ref"][0][[0, 2]], clean["ref"][0][[0, 2]])
        for p in ("pinf1", "pinf2"):
            assert ec.chain_case(K, T, 3, "BTKK", False, p)["ref"][0][1] == ec.INF
        assert np.isnan(ec.chain_case(K, T, 3, "BTKK", False, "nan")["ref"][0][1])
        sh = ec.chain_case(K, T, 3, "BTKK", False, "shift3e4")
        assert np.abs(sh["ref"][0] - clean["ref"][0] - 3e4 * T).max() <= 64 * ec.EPS64 * sh["M"].max()
        assert np.abs(sh["ref"][1] - clean["ref"][1]).max() <= 64 * ec.EPS64 * sh["M"].max()
        hot = ec.chain_case(K, T, 3, "BTKK", False, "scale1e4")["ref"][1]
        assert (hot.max(-1) > 1 - 1e-9).all()                    # one-hot posteriors


def test_chain_grid_reaches_every_body():
    seen = set()
    for f32 in (True, False):
        for K, T in ec.chain_grid(f32) + ec.chain_pattern_shapes(f32):
            body, D = ec.chain_body(K, T, f32)
            seen.add((body, D, f32))
            if D:                                  # a step count on either side of the prefetch depth
                assert {T2 - 1 <= D for T2 in ec.chain_T(K, f32)} == {True, False}
    assert seen == {("lanes16", 8, True), ("lanes16", 8, False), ("lanes32", 4, True), ("lanes32", 2, False),
                    ("generic", 0, True), ("generic", 0, False)}


@pytest.mark.parametrize("name", ec.lse_names())
def test_lse_reference_against_the_oracle(name):
    c = ec.lse_case(name, False)
    terms = [ec.lse_view(t).numpy() for t in c["terms"]]
    with np.errstate(all="ignore"):
        out, _ = o_lse.logsumexp_terms(terms, c["frame"], c["rdim"])
        G = o_lse.logsumexp_terms_grad(terms, c["frame"], c["rdim"], c["g_out"].numpy())
    assert _close(out, c["out"], c["M"])
    assert _close(G, c["G"], c["MG"])
    assert np.isneginf(c["out"]).any() or name in ("cancel",)


def _lda_grid(f32):
    g = []
    for route in ec.LDA_ROUTES:
        g += [(T, V, B, Wd, None, False) for T, V, B, Wd, *_ in ec.lda_cell_cases(route, f32)]
    g += [(8, 50, B, Wd, None, False) for B, Wd in ec.LDA_SIZES]
    g += [(T, V, 70, 5, p, False) for T, V in ec.LDA_PATTERN_SHAPES for p in ec.LDA_PATTERNS + ("impossible_doc_clean",)]
    g += [(8, 7, 300, 8, None, True), (5, 7, 300, 8, None, True)]
    return sorted(set(g), key=str)


def test_lda_reference_against_the_oracle():
    for T, V, B, Wd, pat, ms in _lda_grid(False):
        c = ec.lda_case(T, V, B, Wd, False, pat, ms)
        with np.errstate(all="ignore"):
            got = o_lda.lda_factor(c["words"].numpy(), c["lt"].numpy(), c["lp"].numpy())
        for g, r, M in zip(got, c["ref"], c["M"]):
            assert _close(g, r, M), (T, V, B, Wd, pat)


def test_lda_reference_properties():
    T, V = ec.LDA_PATTERN_SHAPES[0]
    d, v2 = 70 // 2, V - 2
    bad = ec.lda_case(T, V, 70, 5, False, "impossible_doc")
    clean = ec.lda_case(T, V, 70, 5, False, "impossible_doc_clean")
    out, gt, gp = bad["ref"]
    assert out[d] == -ec.INF and (gp[:, v2] == 0).all() and abs(gt[d].sum() - 4) < 1e-12
    others = np.arange(70) != d
    assert np.array_equal(out[others], clean["ref"][0][others])
    assert np.array_equal(gt[others], clean["ref"][1][others])
    base = ec.lda_case(T, V, 70, 5, False)
    sh = ec.lda_case(T, V, 70, 5, False, "shift1e3")
    c = np.where(np.arange(70) % 2 == 0, 1e3, -1e3)
    assert np.abs(sh["ref"][0] - base["ref"][0] - 5 * c).max() <= 64 * ec.EPS64 * sh["M"][0].max()
    assert np.abs(sh["ref"][1] - base["ref"][1]).max() <= 64 * ec.EPS64 * sh["M"][0].max()
    ms = ec.lda_case(8, 7, 300, 8, False, None, True)
    assert (ms["words"] == 0).sum() > ec.LDA_SEG                 # word 0 spans more than one task


@pytest.mark.parametrize("route", ec.LDA_ROUTES)
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_lda_cell_table(route, f32):
    """Every (TMAX, NW, tier) cell the grid names is the one the restated budget formulas produce for
    its (T, V), V + 1 falls in the next cell, and every reachable cell is named."""
    esz = 4 if f32 else 8
    named = set()
    for T, V, B, Wd, tmax, nw, tier in ec.lda_cell_cases(route, f32):
        assert ec.lda_tmax(T) == tmax and T in ec.LDA_T
        assert ec.lda_waves(route, V, tmax, esz) == (nw, tier)
        assert ec.lda_waves(route, V + 1, tmax, esz) != (nw, tier)
        named.add((tmax, nw, tier))
    reachable = {(tmax,) + ec.lda_waves(route, V, tmax, esz) for tmax in (8, 16, 32, 64) for V in range(1, 6000)}
    assert named == {c for c in reachable if c[1]}
    for T, V in ec.lda_refusals(route, f32):
        assert T > 64 or (ec.lda_waves(route, V, ec.lda_tmax(T), esz)[0] == 0 and
                          ec.lda_waves(route, V - 1, ec.lda_tmax(T), esz)[0] > 0)
    assert {ec.lda_tmax(c[0]) for c in ec.lda_cell_cases(route, f32)} == {8, 16, 32, 64}
    if route == "atomic" and not f32:              # the worked example of csrc/lda.hip's formula
        assert [c[3] for c in ec.lda_cells(route, f32) if c[0] == 16] == [96, 368, 504, 572, 606, 607]


def test_unscored_cap_holds_for_every_f32_case():
    """cpu32 alone: at most 5 % of a float32 case's finite reference elements have a non-finite float32
    torch value (those are not scored)."""
    worst = 0.0
    for K, T in ec.chain_grid(True):
        for B in ec.CHAIN_B:
            for lay in ec.CHAIN_LAYOUTS if T > 1 else ("BTKK",):
                c = ec.chain_case(K, T, B, lay, True)
                worst = max([worst] + [ec.unscored_fraction(r, x) for r, x in zip(c["ref"], c["cpu32"])])
    for K, T in ec.chain_pattern_shapes(True):
        for p in ec.CHAIN_PATTERNS:
            c = ec.chain_case(K, T, 3, "BTKK", True, p)
            ok = np.isfinite(c["ref"][0]) | (c["ref"][0] == -ec.INF)
            worst = max([worst] + [ec.unscored_fraction(r[ok], x[ok]) for r, x in zip(c["ref"], c["cpu32"])])
    for name in ec.lse_names():
        c = ec.lse_case(name, True)
        worst = max(worst, ec.unscored_fraction(c["out"], c["cpu32"][0]), ec.unscored_fraction(c["G"], c["cpu32"][1]))
    for T, V, B, Wd, pat, ms in _lda_grid(True):
        c = ec.lda_case(T, V, B, Wd, True, pat, ms)
        worst = max([worst] + [ec.unscored_fraction(r, x) for r, x in zip(c["ref"], c["cpu32"])])
    assert worst <= ec.UNSCORED_CAP, worst


def test_rule_rejects_what_it_should():
    """The scoring helper itself: a transposed xi, a NaN where the reference is finite and a wrong
    non-finite value fail; the reference passes."""
    c = ec.chain_case(3, 4, 3, "BTKK", True)
    ec.chain_check("selftest", c["ref"], c, True)
    with pytest.raises(AssertionError):
        ec.chain_check("selftest", (c["ref"][0], c["ref"][1], c["ref"][2].swapaxes(-1, -2)), c, True)
    d = ec.chain_case(3, 4, 3, "BTKK", False, "dead_batch")
    lz = d["ref"][0].copy()
    lz[1] = ec.NAN
    with pytest.raises(AssertionError):
        ec.chain_check("selftest", (lz,) + d["ref"][1:], d, False)
    # a dropped segment of the multi-segment word: word 0's column of g_phi short of the pairs past LDA_SEG
    m = ec.lda_case(8, 7, 300, 8, True, None, True)
    n0 = int((m["words"] == 0).sum())
    gp = m["ref"][2].copy()
    gp[:, 0] *= ec.LDA_SEG / n0
    with pytest.raises(AssertionError):
        ec.lda_check("selftest", (m["ref"][0], m["ref"][1], gp), m, True)
    ec.RATIOS.pop("selftest", None)
