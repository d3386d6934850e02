"""The three enumeration kernels (pa_logchain_fwd_bwd, pa_logsumexp_terms / _grad, pa_lda_factor_fwd_bwd
/ _indexed_fwd_bwd) on every launch path and at the edges, against the float64 references and under
the one tolerance rule of tests/enum_edge_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import enum_edge_cases as ec

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(True, id="f32"), pytest.param(False, id="f64")]


def _k():
    from pyro_amd import kernels
    return kernels


def _dt(f32):
    return torch.float32 if f32 else torch.float64


def _cpu(xs):
    return tuple(x.double().cpu().numpy() for x in xs)


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    """Prints the largest error / bound per kernel, path and dtype of the module's run (the table of
    tests/enum_edge_cases.py's docstring); PYRO_AMD_ENUM_EDGE_RATIOS names a file to write it to."""
    yield
    table = ec.ratio_table()
    print("\nerror / bound, largest per path:\n" + table)
    path = os.environ.get("PYRO_AMD_ENUM_EDGE_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write(table + "\n")


# ---- chain -------------------------------------------------------------------------------------------

def _chain_run(c, f32, gpu):
    k = _k()
    U, P = c["U"].to(gpu, _dt(f32)).contiguous(), c["P"].to(gpu, _dt(f32)).contiguous()
    return k.logchain_fwd_bwd(U, P)


def _chain_label(K, T, f32):
    body, D = ec.chain_body(K, T, f32)
    return "chain/%s%s/%s" % (body, "_D%d" % D if D else "", "f32" if f32 else "f64")


def _chain_grid_params():
    seen = []
    for f32 in (True, False):
        seen += [pytest.param(K, T, f32, id="K%d-T%d-%s" % (K, T, "f32" if f32 else "f64"))
                 for K, T in ec.chain_grid(f32)]
    return seen


@pytest.mark.parametrize("K,T,f32", _chain_grid_params())
def test_chain_grid(gpu, K, T, f32):
    """Every K around the bodies' limits, every T around the body's prefetch depth, B = 1 and 3, the
    three pairwise layouts ([B,T-1,K,K], [T-1,K,K] and the time-homogeneous [K,K])."""
    for B in ec.CHAIN_B:
        for layout in ec.CHAIN_LAYOUTS if T > 1 else ("BTKK",):
            c = ec.chain_case(K, T, B, layout, f32)
            ec.chain_check(_chain_label(K, T, f32), _cpu(_chain_run(c, f32, gpu)), c, f32)


def _chain_pattern_params():
    out = []
    for f32 in (True, False):
        out += [pytest.param(K, T, f32, p, id="K%d-T%d-%s-%s" % (K, T, "f32" if f32 else "f64", p))
                for K, T in ec.chain_pattern_shapes(f32) for p in ec.CHAIN_PATTERNS]
    return out


@pytest.mark.parametrize("K,T,f32,pattern", _chain_pattern_params())
def test_chain_patterns(gpu, K, T, f32, pattern):
    """-inf unaries, dead ends and unreachable states, a batch element with logZ = -inf, potentials
    times 1e4, a +3e4 shift, a NaN and +inf potentials, on one small and one prefetch-boundary shape per
    body.  A poisoned batch element leaves the others bit-identical to the run without it."""
    c = ec.chain_case(K, T, 3, "BTKK", f32, pattern)
    got = _chain_run(c, f32, gpu)
    ec.chain_check(_chain_label(K, T, f32), _cpu(got), c, f32, pattern)
    lz = got[0].cpu()
    if pattern == "dead_batch":
        assert lz[1] == -ec.INF and (got[1][1] == 0).all() and (got[2][1] == 0).all()
    if pattern == "nan":
        assert torch.isnan(lz[1])
    if pattern in ("pinf1", "pinf2"):
        assert lz[1] == ec.INF                    # as torch.logsumexp of the path scores, on every body
    if ec.chain_clean_of(pattern):
        clean = _chain_run(ec.chain_case(K, T, 3, "BTKK", f32), f32, gpu)
        for a, b in zip(got, clean):
            assert torch.equal(a[[0, 2]], b[[0, 2]])


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("pattern", ["pinf1", "pinf2"])
def test_chain_pinf_is_the_same_on_every_body(gpu, f32, pattern):
    """The same K = 16 chain on the lanes body and embedded in K = 33 (generic body) with the 17 extra
    states out of reach: logZ = +inf for the poisoned element on both, and the clean elements agree
    within the rule.  The extra states sit at -1e30, not -inf: a path through a +inf potential and a
    -inf one scores inf - inf, NaN already in the sum over paths."""
    K, K2, T = 16, 33, 9
    c = ec.chain_case(K, T, 3, "BTKK", f32, pattern)
    U2 = torch.full((3, T, K2), -1e30, dtype=torch.float64)
    P2 = torch.full((3, T - 1, K2, K2), -1e30, dtype=torch.float64)
    U2[:, :, :K] = c["U"]
    P2[:, :, :K, :K] = c["P"]
    small = _cpu(_chain_run(c, f32, gpu))
    big = _cpu(_chain_run({"U": U2, "P": P2}, f32, gpu))
    assert small[0][1] == ec.INF and big[0][1] == ec.INF
    emb = (big[0], big[1][:, :, :K], big[2][:, :, :K, :K])
    ec.chain_check(_chain_label(K2, T, f32), emb, c, f32, pattern)
    assert (big[1][[0, 2]][:, :, K:] == 0).all()


@pytest.mark.parametrize("f32", DTYPES)
def test_chain_refuses_65_states(gpu, f32):
    from pyro_amd import _lib
    U = torch.zeros(2, 3, 65, dtype=_dt(f32), device=gpu)
    P = torch.zeros(2, 65, 65, dtype=_dt(f32), device=gpu)
    with pytest.raises(_lib.Unsupported):
        _k().logchain_fwd_bwd(U, P)


# ---- logsumexp_terms ---------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("name", ec.lse_names())
def test_lse_grid(gpu, name, f32):
    """Kept extent 255 / 256 / 257 (one thread per kept element, 256 per block), reduced extent 1 / 2 /
    1000, rdim first / middle / last; PA_LSE_MAX_TERMS terms over PA_LSE_MAX_DIMS dims; a transposed and
    a stride-0 term read through their own strides; terms that cancel at 1e4."""
    k = _k()
    c = ec.lse_case(name, f32)
    terms = []
    for t in c["terms"]:
        base = (t[0] if isinstance(t, tuple) else t).to(gpu, _dt(f32)).contiguous()
        terms.append(ec.lse_view((base, t[1])) if isinstance(t, tuple) else base)
    if name == "strided":
        assert not terms[0].is_contiguous() and 0 in terms[1].stride()
    out = k.logsumexp_terms(terms, c["frame"], c["rdim"])
    G = k.logsumexp_terms_grad(terms, c["frame"], c["rdim"], out, c["g_out"].to(gpu, _dt(f32)))
    ec.lse_check("lse/%s" % ("f32" if f32 else "f64"), *_cpu((out, G)), c, f32)


# ---- lda factor --------------------------------------------------------------------------------------

def _lda_run(c, f32, route, gpu):
    k = _k()
    words = c["words"].to(gpu).contiguous()
    lt, lp = c["lt"].to(gpu, _dt(f32)).contiguous(), c["lp"].to(gpu, _dt(f32)).contiguous()
    if route == "indexed":
        index = k.lda_build_index(words, lp.shape[1])
        assert index is not None
        return k.lda_factor_fwd_bwd(words, lt, lp, index=index)
    k.lda_set_index_mode(k.LDA_INDEX_OFF)
    try:
        return k.lda_factor_fwd_bwd(words, lt, lp)
    finally:
        k.lda_set_index_mode(k.LDA_INDEX_AUTO)


def _lda_cell_params():
    out = []
    for route in ec.LDA_ROUTES:
        for f32 in (True, False):
            for T, V, B, Wd, tmax, nw, tier in ec.lda_cell_cases(route, f32):
                out.append(pytest.param(route, f32, T, V, B, Wd, id="%s-%s-TMAX%d-NW%d-%dK-T%d-V%d" % (
                    route, "f32" if f32 else "f64", tmax, nw, tier, T, V)))
    return out


@pytest.mark.parametrize("route,f32,T,V,B,Wd", _lda_cell_params())
def test_lda_cells(gpu, route, f32, T, V, B, Wd):
    """One launch per reachable (TMAX, NW, dtype, route) instantiation, at the largest V of the cell
    (tests/enum_edge_cases.py::lda_cells restates the two LDS budget formulas)."""
    c = ec.lda_case(T, V, B, Wd, f32)
    label = "lda/%s/TMAX%d/%s" % (route, ec.lda_tmax(T), "f32" if f32 else "f64")
    ec.lda_check(label, _cpu(_lda_run(c, f32, route, gpu)), c, f32)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("route", ec.LDA_ROUTES)
def test_lda_refusals(gpu, route, f32):
    """T = 65 and the first V whose tables do not fit in LDS raise Unsupported (the wrapper has no
    fallback)."""
    from pyro_amd import _lib
    for T, V in ec.lda_refusals(route, f32):
        c = ec.lda_case(T, V, 3, 2, f32)
        with pytest.raises(_lib.Unsupported):
            _lda_run(c, f32, route, gpu)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("route", ec.LDA_ROUTES)
def test_lda_sizes(gpu, route, f32):
    """B = 1, 64, 65, 70 (a ragged last tile of 64 documents) and Wd = 0, 1, 5."""
    for B, Wd in ec.LDA_SIZES:
        c = ec.lda_case(8, 50, B, Wd, f32)
        ec.lda_check("lda/%s/TMAX8/%s" % (route, "f32" if f32 else "f64"), _cpu(_lda_run(c, f32, route, gpu)), c, f32)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("T", [8, 5])
def test_lda_multi_segment_word(gpu, T, f32):
    """Indexed route: word 0 holds more than LDA_SEG pairs, its list spans several tasks and the
    finalize kernel sums the segments; g_phi is bitwise equal on a second call."""
    c = ec.lda_case(T, 7, 300, 8, f32, None, True)
    assert int((c["words"] == 0).sum()) > ec.LDA_SEG
    got = _lda_run(c, f32, "indexed", gpu)
    ec.lda_check("lda/indexed/TMAX8/%s" % ("f32" if f32 else "f64"), _cpu(got), c, f32)
    again = _lda_run(c, f32, "indexed", gpu)
    assert torch.equal(got[2], again[2]) and torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("route", ec.LDA_ROUTES)
@pytest.mark.parametrize("TV", ec.LDA_PATTERN_SHAPES, ids=lambda tv: "T%d-V%d" % tv)
@pytest.mark.parametrize("pattern", ec.LDA_PATTERNS)
def test_lda_patterns(gpu, pattern, TV, route, f32):
    """A topic absent from a document, a word impossible under one topic, a document with a word
    impossible under all of its topics, per-document shifts of +-1e3."""
    T, V = TV
    c = ec.lda_case(T, V, 70, 5, f32, pattern)
    got = _lda_run(c, f32, route, gpu)
    label = "lda/%s/TMAX%d/%s" % (route, ec.lda_tmax(T), "f32" if f32 else "f64")
    ec.lda_check(label, _cpu(got), c, f32)
    if pattern == "impossible_doc":
        d, v2 = 70 // 2, V - 2
        assert got[0][d] == -ec.INF and (got[2][:, v2] == 0).all()       # the pair contributes exactly 0
        clean = _lda_run(ec.lda_case(T, V, 70, 5, f32, "impossible_doc_clean"), f32, route, gpu)
        others = torch.arange(70, device=gpu) != d
        assert torch.equal(got[0][others], clean[0][others]) and torch.equal(got[1][others], clean[1][others])
    if pattern == "shift1e3":
        base = ec.lda_case(T, V, 70, 5, f32)
        sign = np.where(np.arange(70) % 2 == 0, 1e3, -1e3)
        shifted = dict(base, ref=(base["ref"][0] + 5 * sign,) + base["ref"][1:], M=c["M"], cpu32=c["cpu32"])
        # out shifts by Wd c, the responsibilities are those of the unshifted corpus (f32 inputs are rounded
        # after the shift: the f64 reference of the shifted inputs above is the exact statement there)
        if not f32:
            ec.lda_check(label, _cpu(got), shifted, f32)
