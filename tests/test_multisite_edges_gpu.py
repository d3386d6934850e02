"""The many-small-sites kernels -- pa_multi_log_prob_sum / _grad / _sum_grad, pa_meanfield_normal_sample / _bwd and
the chained tail that runs them with Adam as phases of one launch -- per element against the float64 references and
under the tolerance rule of tests/multisite_edge_cases.py, on every launch path and at the borders between them,
with NaN-filled canaries around every input and sentinel-filled ones around every output of a direct C-ABI call."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import philox as o_philox
from tests import dist_edge_cases as ec
from tests import multisite_edge_cases as mc
from tests.test_guide_edges_gpu import FILL, PAD, Carved, _bits_equal

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(True, id="f32"), pytest.param(False, id="f64")]
NAN = float("nan")


def _k():
    from pyro_amd import kernels
    return kernels


def _lib():
    from pyro_amd import _lib
    return _lib


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


class Guarded(Carved):
    """Carved with a chosen canary: NaN around the inputs, True around a mask."""

    def __init__(self, shape, f32, gpu, init=None, dtype=None, fill=NAN):
        super().__init__(shape, f32, gpu, init, dtype)
        self.fill = fill
        self.big[:PAD] = fill
        self.big[PAD + self.n:] = fill

    def intact(self):
        edge = torch.cat([self.big[:PAD], self.big[PAD + self.n:]])
        if isinstance(self.fill, float) and math.isnan(self.fill):
            return bool(torch.isnan(edge).all())
        return bool((edge == self.fill).all())


def _upload(t, f32, gpu):
    """A CPU tensor (any 2-D view of its storage) -> (guard, the same view of a guarded copy of the storage)."""
    if t.dtype == torch.bool:
        g = Guarded(tuple(t.shape), f32, gpu, t.contiguous(), dtype=torch.bool, fill=True)
        return g, g.t
    n = t.untyped_storage().nbytes() // t.element_size()
    whole = torch.as_strided(t, (n,), (1,), 0)
    g = Guarded((n,), f32, gpu, whole)
    return g, torch.as_strided(g.t, tuple(t.shape), t.stride(), g.t.storage_offset() + t.storage_offset())


# =======================================================================================================
# the assembly through the C ABI
# =======================================================================================================

class Table:
    """One launch's entry table on guarded device buffers; gradient outputs carved and pre-filled with FILL."""

    def __init__(self, ents, f32, gpu, shared=None):
        k, lib = _k(), _lib()
        self.guards, self.outs, self.untouched = [], [], []
        self.dev = {} if shared is None else shared            # id(CPU tensor) -> device view: chains share a value
        self.arr = (lib.SiteEntry * max(len(ents), 1))()
        for i, e in enumerate(ents):
            R, C = e["rows"], e["cols"]
            views, srcs = [], []
            for key in ("value", "p0", "p1", "mask"):
                t = e[key]
                if t is not None and id(t) not in self.dev:
                    g, v = _upload(t, f32, gpu)
                    self.guards.append(g)
                    self.dev[id(t)] = v
                srcs.append(None if t is None else self.dev[id(t)])
                views.append(k._view(srcs[-1], R, C))
            outs, bits = [], 0
            by_chain = bool(e.get("by_chain"))
            for j in range(3):
                if e["need"][j] and srcs[j] is not None and not (j == 0 and by_chain):
                    o = Carved(k._reduced_shape(views[j], R, C), f32, gpu)
                    self.guards.append(o)
                    outs.append(o.t)
                    bits |= 1 << j
                else:
                    outs.append(None)
            if by_chain:
                bits |= lib.NEED_VALUE | lib.VALUE_BY_CHAIN
            d_p1 = outs[2]
            if e.get("force_p1"):                   # need set for the p1 a one-parameter family does not have
                o = Carved((R, C), f32, gpu)
                self.guards.append(o)
                self.untouched.append(o)
                bits |= lib.NEED_P1
                d_p1 = o.t
            xg = e.get("extra_grad")
            if xg is not None:
                g, xg = _upload(xg.reshape(R, C), f32, gpu)
                self.guards.append(g)
            self.arr[i] = lib.SiteEntry(e["dist"], bits, R, C, views[0], views[1], views[2], views[3], float(e["coef"]),
                                        k._ptr(outs[0]), k._ptr(outs[1]), k._ptr(d_p1), int(e.get("chain_next", -1)), 0,
                                        k._ptr(xg), float(e.get("extra_coef", 0.0)))
            self.outs.append(tuple(outs))
        self.n = len(ents)

    def verify(self):
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.guards), "a canary next to a buffer of the assembly was overwritten"
        for o in self.untouched:
            assert bool((o.t == FILL).all()), "d_p1 of a one-parameter family was written"

    def grads(self):
        return [tuple(_np(x) for x in row) for row in self.outs]


def _run(ents, coef_all, g, f32, gpu, mode):
    """mode "grad" / "sum" / "sum_grad" on chunks of 16 entries (later chunks accumulate into the total, as the
    wrapper launches them) -> (total or None, [(dv, da, db)] numpy or None)."""
    k, lib = _k(), _lib()
    d = k._DTYPES[mc.dt(f32)]
    out = Carved((1,), f32, gpu)
    gt = None if g is None else Guarded((1,), f32, gpu, torch.tensor([g], dtype=torch.float64))
    grads, shared = [], {}
    for lo in range(0, max(len(ents), 1), mc.MAX_ENTRIES):
        tb = Table(ents[lo:lo + mc.MAX_ENTRIES], f32, gpu, shared)
        if mode == "grad":
            rc = lib.load().pa_multi_log_prob_grad(d, k._ptr(gt.t), tb.arr, tb.n, float(coef_all), k._stream())
        elif mode == "sum":
            rc = lib.load().pa_multi_log_prob_sum(d, k._ptr(out.t), tb.arr, tb.n, float(coef_all), int(lo > 0),
                                                  k._stream())
        else:
            rc = lib.load().pa_multi_log_prob_sum_grad(d, k._ptr(out.t), None if gt is None else k._ptr(gt.t), tb.arr,
                                                       tb.n, float(coef_all), int(lo > 0), k._stream())
        k.check(rc)
        tb.verify()
        grads += tb.grads()
    assert out.intact() and (gt is None or gt.intact())
    return (None if mode == "grad" else float(out.t.double().item())), (None if mode == "sum" else grads)


def _assembly(label, ents, coef_all, g, f32, gpu, mode, case=None):
    case = case or mc.assembly_case(ents, coef_all, 1.0 if g is None else g, f32)
    total, grads = _run(ents, coef_all, g, f32, gpu, mode)
    mc.score_assembly(label, case, f32, total, grads)
    return case


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("C", mc.THREAD_MAP_C)
def test_thread_map_of_the_gradient_pass(gpu, C, f32):
    """pa_multi_log_prob_grad on Normal entries: C either side of 32 / 64 / 128 / 256 threads and of two column
    blocks, R at 1, ng, ng + 1, 8 ng and 8 ng + 1 (one batch of UN rows per group, and one row more); every operand
    FULL, and p0 ROWRED with p1 SCALAR (the barrier inside the column-block loop)."""
    _assembly("grad", mc.thread_map_table(C), -0.25, 1.7, f32, gpu, "grad")


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("frame", mc.PATTERN_FRAMES, ids=lambda f: "%dx%d" % f)
def test_operand_patterns(gpu, frame, f32):
    """All 4^3 broadcast patterns of (value, p0, p1) x no mask / [R,C] / [1,C] / [R,1] masks: the combined pass, the
    generic per-operand pass for a reduced value and COLRED parameters, the SCALAR reduction; odd tables through
    pa_multi_log_prob_grad, even ones through pa_multi_log_prob_sum_grad with g given (the total is scored too)."""
    for i, tb in enumerate(mc.pattern_tables(*frame)):
        _assembly("grad", tb, -0.25, 1.7, f32, gpu, "grad" if i % 2 else "sum_grad")


@pytest.mark.parametrize("f32", DTYPES)
def test_degenerate_frames_and_odd_entries(gpu, f32):
    """Frames (1, C), (R, 1) and (1, 1), where a stride-0 dimension of extent 1 is FULL; a transposed and a
    column-sliced value; one-parameter families with need set for p1; identity entries; an entry that asks for no
    gradient; empty entries [0, 4] and [4, 0] (the latter divided by zero in the total's workgroup before
    multi_sum_partial skipped empty entries)."""
    for frame in mc.DEGENERATE_FRAMES:
        for tb in mc.pattern_tables(*frame, masked=False):
            _assembly("grad/degenerate", tb, -0.25, 1.7, f32, gpu, "grad")
    ents = mc.odd_entries_table()
    _assembly("grad/odd", ents, 0.5, 1.7, f32, gpu, "grad")
    _assembly("grad/odd", ents, 0.5, None, f32, gpu, "sum_grad")
    _assembly("grad/odd", ents, 0.5, None, f32, gpu, "sum")
    empty = [e for e in ents if e["rows"] * e["cols"] == 0]
    total, _ = _run(empty, 3.0, None, f32, gpu, "sum")
    assert total == 0.0
    total, grads = _run(empty, 3.0, None, f32, gpu, "sum_grad")
    assert total == 0.0 and all(x.size == 0 for row in grads for x in row)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("n", mc.TOTAL_N)
def test_total(gpu, n, f32):
    """pa_multi_log_prob_sum and the total of pa_multi_log_prob_sum_grad on n entries -- 16, 8, 5, 4, 3, 2 or 1 waves
    per entry; from 17 entries on, accumulating launches -- with C below, at and above the entry's threads, R at
    4 ng - 1, 4 ng, 4 ng + 1, signed coefficients; and every entry alone, so that the scalar cannot hide a misread
    entry."""
    ents = mc.total_table(n)
    wpe = mc.sum_map(1, min(n, 16))[0]
    case = _assembly("sum/wpe%d" % wpe, ents, -0.25, None, f32, gpu, "sum")
    if n <= mc.MAX_ENTRIES:              # (float64: a 256-thread launch, 4 waves for the total's workgroup)
        wpe2 = wpe if f32 else mc.sum_map(1, n, waves=4)[0]
        _assembly("sum_grad/wpe%d" % wpe2, ents, -0.25, None, f32, gpu, "sum_grad", case)
    for e in ents:
        _assembly("sum/alone", [e], -0.25, None, f32, gpu, "sum")


def _chain_tables():
    out = []
    for members in (1, 2, 3):
        for i, frame in enumerate(mc.PATTERN_FRAMES):
            out.append(mc.chain_table(members, frame, (0.5, -2.0, None)[(members + i) % 3], seed=i))
    out.append(mc.two_chains_table())
    return out


@pytest.mark.parametrize("f32", DTYPES)
def test_chains_and_extras(gpu, f32):
    """A Gamma head with 1, 2 and 3 chained members (LogNormal, HalfCauchy, Normal) on one value tensor, the members'
    own p0 / p1 gradients in every pattern, the extra term with extra_coef 0.5 and -2, g = 1.7 through
    pa_multi_log_prob_grad and g = NULL through pa_multi_log_prob_sum_grad; two independent chains in one table, a
    head that is not entry 0, a chain that points backwards.  Every d_value is pre-filled with a sentinel: the head
    overwrites it (an accumulating head would be off by the sentinel)."""
    for ents in _chain_tables():
        _assembly("chain", ents, -0.25, 1.7, f32, gpu, "grad")
        _assembly("chain", ents, -0.25, None, f32, gpu, "sum_grad")
    # the extra term alone moves d_value by exactly g coef_all extra_coef extra_grad
    ents = mc.chain_table(2, (9, 33), 0.5)
    plain = [dict(e) for e in ents]
    plain[0] = dict(plain[0], extra_grad=None)
    _, with_x = _run(ents, -0.25, 1.0, f32, gpu, "grad")
    _, without = _run(plain, -0.25, 1.0, f32, gpu, "grad")
    assert not np.array_equal(with_x[0][0], without[0][0])
    for a, b in zip(with_x[1:], without[1:]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(x, y)


def test_ill_formed_chains_are_refused_before_any_launch(gpu):
    """A chain on a broadcast value, a frame mismatch and chain_next == k: an error code, and nothing written."""
    k, lib = _k(), _lib()
    for why, ents in mc.refusal_tables():
        tb = Table(ents, True, gpu)
        out = Carved((1,), True, gpu)
        g = Guarded((1,), True, gpu, torch.tensor([1.0]))
        for call in (lambda: lib.load().pa_multi_log_prob_grad(k._DTYPES[torch.float32], k._ptr(g.t), tb.arr, tb.n, 1.0,
                                                                k._stream()),
                     lambda: lib.load().pa_multi_log_prob_sum_grad(k._DTYPES[torch.float32], k._ptr(out.t), None, tb.arr,
                                                                    tb.n, 1.0, 0, k._stream()),
                     lambda: lib.load().pa_multi_log_prob_sum(k._DTYPES[torch.float32], k._ptr(out.t), tb.arr, tb.n, 1.0,
                                                               0, k._stream())):
            assert call() == lib.PA_ERR_INVALID, why
        tb.verify()
        assert bool((out.big == FILL).all()), why
        for row in tb.outs:
            for o in row:
                assert o is None or bool((o == FILL).all()), why


@pytest.mark.parametrize("f32", DTYPES)
def test_families_at_the_edges_through_chains(gpu, f32):
    """Every family's edge grid on a [2, n] frame as a masked chain head with a Normal member chained on its value:
    the head's d_value = its own gradient + the member's through the accumulating pass old + w * gv, NaN / inf
    pattern included (float64: exactly the reference's), and the head's parameter gradients."""
    rng = np.random.default_rng(7)
    for dist in sorted(ec.NAMES):
        c = mc.edge_chain_case(dist, f32, rng)
        _, grads = _run(c["entries"], 2.0, None, f32, gpu, "sum_grad")
        c32 = c["cpu32"] or (None, None, None)
        for what, got, ref, M, r32 in zip(("d_value", "d_p0", "d_p1"), grads[0], c["ref"], c["M"], c32):
            if ref is not None:
                mc.score("edges/chain/" + mc.dname(f32), "%s %s" % (ec.NAMES[dist], what), got, ref, M, f32, r32,
                         cap=1.0)      # (dist_edge_cases' grids overflow float32 on purpose: see the cases module)
        assert grads[1] == (None, None, None)


# =======================================================================================================
# the draw
# =======================================================================================================

def _draw(ns, P, f32, gpu, seed=11):
    """pa_meanfield_normal_sample on guarded buffers, site k at Philox offset 1000 k -> per site (z, scale, loc_out,
    eps) tensors and the (loc, rho) float64 inputs."""
    k, lib = _k(), _lib()
    arr = (lib.MfSite * len(ns))()
    guards, outs, params = [], [], []
    shift = 0
    for i, n in enumerate(ns):
        loc, rho = mc.draw_params(n, f32, shift)
        shift += n
        gl, gr = Guarded((n,), f32, gpu, loc), Guarded((n,), f32, gpu, rho)
        o = [Carved(s, f32, gpu) for s in ((P, n), (n,), (n,), (P, n))]
        guards += [gl, gr] + o
        arr[i] = lib.MfSite(k._ptr(gl.t), k._ptr(gr.t), k._ptr(o[0].t), k._ptr(o[1].t), k._ptr(o[2].t), k._ptr(o[3].t),
                            n, 1000 * i, 0, 0, None, None, None, None, None)
        outs.append(tuple(x.t for x in o))
        params.append((loc, rho))
    k.check(lib.load().pa_meanfield_normal_sample(k._DTYPES[mc.dt(f32)], arr, len(ns), P, seed, None, k._stream()))
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), "a canary next to a buffer of the draw was overwritten"
    return outs, params


def _score_draw(label, n, P, out, loc, rho, off, f32):
    z, sc, lo, eps = (_np(x) for x in out)
    tol = 2e-6 if f32 else 1e-13
    ref_eps = o_philox.normal(P * n, np.float32 if f32 else np.float64, 11, off).reshape(P, n)
    np.testing.assert_allclose(eps, ref_eps, rtol=tol, atol=10 * tol)
    assert np.array_equal(lo, loc)
    zr, sr = mc.draw_reference(loc, rho, eps, mc.F64)
    z32, s32 = mc.draw_reference(loc, rho, eps, mc.F32) if f32 else (None, None)
    Mz, Ms = mc.draw_magnitudes(loc, rho, eps)
    mc.score("%s/%s" % (label, mc.dname(f32)), "scale", sc, sr, Ms, f32, s32)
    mc.score("%s/%s" % (label, mc.dname(f32)), "z", z, zr, Mz, f32, z32)


DRAW_SMALL = mc.DRAW_N * 3                 # 12 sites, 39 elements: every (loc, rho) pair of the grid
# per P: sites that put the launch on the block kernel (P n >= 65 536): whole-block rows, and n % 4 != 0 / P = 1
# (the generic loop)
DRAW_BIG = {5: (13108, 13109), 2: (32768, 32770), 1: (65536,)}


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("P", mc.DRAW_P)
def test_draw(gpu, P, f32):
    """rho from -104 (float32 softplus underflows) to 80 either side of the threshold 20, loc 0, +-1e4, 1e-30, sites
    of 1, 3, 4 and 5 elements: on the per-element kernel, and beside a site of 65 536 elements on the block kernel
    (rows of whole Philox blocks: the vector form; n % 4 != 0 or P = 1: the generic loop).  eps is the oracle's
    stream, scale and z follow the rule, and the kernels are bit-equal on the sites they share."""
    small, params = _draw(DRAW_SMALL, P, f32, gpu)
    for i, (n, out, (loc, rho)) in enumerate(zip(DRAW_SMALL, small, params)):
        _score_draw("draw/element", n, P, out, loc, rho, 1000 * i, f32)
    ns = DRAW_SMALL + DRAW_BIG[P]
    assert P * max(ns) >= 65536
    big, params = _draw(ns, P, f32, gpu)
    for a, b in zip(small, big):
        for x, y in zip(a, b):
            assert _bits_equal(x, y), "the block kernel differs from the per-element kernel on a shared site"
    per = 4 if f32 else 2
    for i in range(len(DRAW_SMALL), len(ns)):
        n = ns[i]
        path = "vector" if (n % per == 0 and P >= 2) else "generic"
        _score_draw("draw/block_" + path, n, P, big[i], *params[i], 1000 * i, f32)


# =======================================================================================================
# the backward of the draw
# =======================================================================================================

def _bwd(cases, which, P, f32, gpu, sinks):
    """pa_meanfield_normal_sample_bwd on guarded buffers, one site per case -> [(d_loc, d_rho)] tensors."""
    k, lib = _k(), _lib()
    arr = (lib.MfSite * len(cases))()
    guards, outs = [], []
    for i, c in enumerate(cases):
        inp = c["inp"]
        n = inp["rho"].size
        b = {w: Guarded(inp[w].shape, f32, gpu, inp[w]) for w in ("rho", "eps", "d_z", "d_scale", "d_loc_out")}
        o = [Carved((n,), f32, gpu, torch.full((n,), 1.5) if sinks else None) for _ in range(2)]
        guards += list(b.values()) + o
        arr[i] = lib.MfSite(None, k._ptr(b["rho"].t), None, None, None, k._ptr(b["eps"].t), n, 0, int(sinks), 0,
                            k._ptr(b["d_z"].t) if which[0] else None, k._ptr(b["d_scale"].t) if which[1] else None,
                            k._ptr(b["d_loc_out"].t) if which[2] else None, k._ptr(o[0].t), k._ptr(o[1].t))
        outs.append((o[0].t, o[1].t))
    k.check(lib.load().pa_meanfield_normal_sample_bwd(k._DTYPES[mc.dt(f32)], arr, len(cases), P, k._stream()))
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), "a canary next to a buffer of the backward was overwritten"
    return outs


ALL3 = (True, True, True)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("n", mc.BWD_N)
def test_backward_of_the_draw(gpu, n, f32):
    """n either side of 256 (one column tile) and of 4096 (64-column tiles x 4 row groups from P = 16 on), P at
    1, 8 ng - 1, 8 ng, 8 ng + 1 (one batch of UN particles per group, and one more), 15 and 16; rho around 20;
    plain outputs and sinks holding 1.5; every None-combination of (d_z, d_scale, d_loc_out) at P = 8 ng + 1 and 16;
    a repeated launch is bit-equal."""
    ng = mc.bwd_map(n, 1)[1]
    for P in mc.bwd_P(n):
        combos = mc.WHICH if P in (8 * ng + 1, 16) else (ALL3,)
        for which in combos:
            c = mc.bwd_case(n, P, which, f32)
            (plain,) = _bwd([c], which, P, f32, gpu, sinks=False)
            mc.score_bwd("bwd", tuple(_np(x) for x in plain), c, f32)
            (acc,) = _bwd([c], which, P, f32, gpu, sinks=True)
            mc.score_bwd("bwd/sinks", tuple(_np(x) for x in acc), c, f32, add=1.5)
        (again,) = _bwd([c], which, P, f32, gpu, sinks=False)
        assert _bits_equal(plain[0], again[0]) and _bits_equal(plain[1], again[1])


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("P", [5, 16])
def test_backward_of_16_and_17_sites(gpu, P, f32):
    """16 sites in one launch (the table's capacity) with a 4097-column site among small ones -- at P = 16 the
    launch's grid is sized for 64-column tiles while the small sites keep their own map -- and 17 sites through the
    wrapper, which launches 16 + 1."""
    k = _k()
    ns = [1, 2, 32, 33, 255, 256, 257, 4097, 3, 64, 65, 128, 129, 5, 7, 300, 31]
    cases = [mc.bwd_case(n, P, ALL3, f32, seed=i) for i, n in enumerate(ns)]
    for sinks in (False, True):
        outs = _bwd(cases[:16], ALL3, P, f32, gpu, sinks)
        for c, o in zip(cases, outs):
            mc.score_bwd("bwd/16sites", tuple(_np(x) for x in o), c, f32, add=1.5 if sinks else 0.0)
    d = mc.dt(f32)
    t = lambda w: [torch.tensor(c["inp"][w], dtype=d, device=gpu) for c in cases]   # noqa: E731
    d_locs, d_rhos = k.meanfield_normal_sample_bwd(t("rho"), t("eps"), t("d_z"), t("d_scale"), t("d_loc_out"), P)
    assert len(d_locs) == 17
    for c, a, b, o in zip(cases, d_locs, d_rhos, outs + [None]):
        mc.score_bwd("bwd/17sites", (_np(a), _np(b)), c, f32)
    again = _bwd(cases[:16], ALL3, P, f32, gpu, False)
    for (a, b), x, y in zip(again, d_locs, d_rhos):
        assert _bits_equal(a, x) and _bits_equal(b, y)


# =======================================================================================================
# the whole tail in its four forms
# =======================================================================================================
FORMS = ("separate", "phases", "fused", "fast")
COEF_ALL = -1.0 / 16


def _tail(form, sites, inp, P, xcoef, clipped, zero_grad, f32, gpu):
    """One step's tail built by hand with the wrappers: the draw from views of one flat parameter buffer, per site a
    prior head entry and a chained by-chain Normal guide entry, multi_log_prob_sum_grad, the draw's backward into
    slices that tile the flat gradient buffer, adam_step on the flat buffers.  ``form``: separate launches, or a
    recorded chain launched phase by phase / fused / fused with the one-pass site code."""
    k = _k()
    d = mc.dt(f32)
    N = inp["p"].size
    flat = {w: Carved((N,), f32, gpu, inp[w]) for w in "pgmv"}
    step = Carved((2,), f32, gpu, [mc.TAIL_STEP0, 0], dtype=torch.int64)
    locs = [flat["p"].t[o:o + n] for o, n in inp["locs"]]
    rhos = [flat["p"].t[o:o + n] for o, n in inp["rhos"]]
    zs, scales, louts, epss = k.meanfield_normal_sample(locs, rhos, P, 11, [1000 * i for i in range(len(sites))])
    dev = lambda x: None if x is None else x.to(gpu) if x.dtype == torch.bool else x.to(gpu, d)   # noqa: E731
    ents = []
    for i, (s, z, sc, lo) in enumerate(zip(sites, zs, scales, louts)):
        n, prior, p0, p1, m = s
        fr = (1, P) if n == 1 else (P, n)
        ents.append(dict(dist=prior, rows=fr[0], cols=fr[1], value=z.view(fr), p0=dev(p0), p1=dev(p1), mask=dev(m),
                         coef=1.0, need=(True, False, False), chain_next=2 * i + 1,
                         extra_grad=None if xcoef is None else torch.tensor(inp["extra"][i], dtype=d, device=gpu),
                         extra_coef=0.0 if xcoef is None else xcoef))
        ents.append(dict(dist=0, rows=fr[0], cols=fr[1], value=z.view(fr), p0=lo.view(1, n), p1=sc.view(1, n),
                         mask=None, coef=-1.0, need=(True, True, True), by_chain=True))
    sinks = [(flat["g"].t[o:o + n], flat["g"].t[o2:o2 + n]) for (o, n), (o2, _) in zip(inp["locs"], inp["rhos"])]
    hy = dict(mc.TAIL_HYPER) if clipped else dict(mc.TAIL_HYPER, clip=0.0, lrd=1.0)
    torch.cuda.synchronize()

    def body():
        total, grads = k.multi_log_prob_sum_grad(ents, COEF_ALL, d, gpu)
        nk = range(len(sites))
        k.meanfield_normal_sample_bwd(rhos, epss, [grads[2 * i][0] for i in nk], [grads[2 * i + 1][2] for i in nk],
                                      [grads[2 * i + 1][1] for i in nk], P, sinks=sinks)
        k.adam_step(flat["p"].t, flat["g"].t, flat["m"].t, flat["v"].t, step.t, lr=hy["lr"], betas=hy["betas"],
                    eps=hy["eps"], weight_decay=hy["wd"], clip_norm=hy["clip"], lrd=hy["lrd"], clipped=clipped,
                    zero_grad=zero_grad)
        return total, grads

    rec = None
    if form == "separate":
        total, grads = body()
    else:
        k.chain_tune(fuse_tail=form in ("fused", "fast"), fast_sites=form == "fast")
        try:
            with k.chain_recording(gpu) as rec:
                total, grads = body()
        finally:
            k.chain_tune(fuse_tail=True)
    torch.cuda.synchronize()
    assert all(x.intact() for x in flat.values()) and step.intact(), "a canary next to a flat buffer was overwritten"
    assert step.t.tolist() == [mc.TAIL_STEP0 + 1, 0]
    out = dict(total=total, p=flat["p"].t, m=flat["m"].t, v=flat["v"].t, left=flat["g"].t,
               d_value=[grads[2 * i][0].reshape(P, s[0]) for i, s in enumerate(sites)],
               d_guide=[x for i in range(len(sites)) for x in grads[2 * i + 1][1:]], eps=epss)
    return out, rec


def _score_tail(label, got, sites, inp, P, xcoef, clipped, zero_grad, f32):
    eps = [_np(e) for e in got["eps"]]
    ref = mc.tail_reference(sites, inp, eps, P, COEF_ALL, xcoef, clipped, mc.F64)
    c32 = mc.tail_reference(sites, inp, eps, P, COEF_ALL, xcoef, clipped, mc.F32) if f32 else None
    M = mc.tail_magnitudes(sites, inp, eps, P, COEF_ALL, xcoef, ref, clipped)
    lab = "%s/%s" % (label, mc.dname(f32))
    get = lambda w: None if c32 is None else c32[w]   # noqa: E731
    nent = 2 * len(sites)
    k_tot = max(mc.k_sum(*((1, P) if s[0] == 1 else (P, s[0])), nent) for s in sites)
    mc.score(lab, "total", np.float64(got["total"].double().item()), ref["total"], M["total"], f32, get("total"),
             k=k_tot)
    for i in range(len(sites)):
        mc.score(lab, "d_value %d" % i, _np(got["d_value"][i]), ref["d_value"][i], M["d_value"][i], f32,
                 None if c32 is None else c32["d_value"][i])
    kg = np.zeros(inp["p"].size)
    for (o, n), (o2, _), kk in zip(inp["locs"], inp["rhos"], mc.tail_k(sites, P)):
        kg[o:o + n] = kk
        kg[o2:o2 + n] = kk
    if zero_grad:
        assert bool((got["left"] == 0).all())
    else:
        for kk in sorted(set(kg.tolist())):
            sel = kg == kk
            mc.score(lab, "gradient", _np(got["left"])[sel], ref["grad"][sel], M["grad"][sel], f32,
                     None if c32 is None else c32["grad"][sel], k=kk)
    for w, what in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        mc.score(lab, what, _np(got[w]), ref[w], M[w], f32, get(w))


def _tail_config(shapes, P, seed, priors=None, masked=None, xcoef=0.5, clipped=False, zero_grad=True):
    sites = mc.tail_sites(shapes, P, seed, priors, masked)
    return dict(sites=sites, P=P, inp=mc.tail_inputs(sites, P, clipped, seed), xcoef=xcoef, clipped=clipped,
                zero_grad=zero_grad,
                fast=sum(mc.fast_site_expected(s[0], P, s[1], s[4] is not None) for s in sites))


def _tail_configs():
    c = []
    # COLS, eligible: (2, 64), (32, 64), (33, 56), (128, 16), (129, 8), (256, 8); SCALAR at P = 2, 63, 64
    c.append(("cols_P64", _tail_config((2, 32, 1), 64, 1, xcoef=0.5, clipped=False, zero_grad=True)))
    c.append(("cols_P56", _tail_config((33,), 56, 2, xcoef=None, clipped=True, zero_grad=False)))
    c.append(("cols_P16", _tail_config((128,), 16, 3, xcoef=-2.0, clipped=False, zero_grad=False)))
    c.append(("cols_P8", _tail_config((129, 256, 257), 8, 4, xcoef=0.5, clipped=True, zero_grad=True)))
    c.append(("scalar_P63", _tail_config((1,), 63, 5, xcoef=0.5, clipped=False, zero_grad=False)))
    c.append(("scalar_P2", _tail_config((1, 2), 2, 6, xcoef=None, clipped=False, zero_grad=True)))
    # just past the border: (32, 65), (33, 57), (129, 9), (257, 8) above, SCALAR at P = 1 and 65
    c.append(("past_P65", _tail_config((32, 1), 65, 7, xcoef=0.5, clipped=False, zero_grad=False)))
    c.append(("past_P57", _tail_config((33,), 57, 8, xcoef=0.5, clipped=True, zero_grad=True)))
    c.append(("past_P9", _tail_config((129,), 9, 9, xcoef=None, clipped=False, zero_grad=False)))
    c.append(("past_P1", _tail_config((1,), 1, 10, xcoef=0.5, clipped=False, zero_grad=True)))
    # 8 sites, a masked head and a Gamma prior among them (both generic inside the fused form)
    c.append(("eight", _tail_config((3, 5, 16, 32, 7, 1, 4, 2), 8, 11, priors=(0, 0, 6, 0, 0, 0, 0, 0),
                                    masked=(False, True, False, False, False, False, False, False), xcoef=-2.0,
                                    clipped=True, zero_grad=False)))
    return c


TAIL_CONFIGS = _tail_configs()
TAIL_FAST = {"cols_P64": 3, "cols_P56": 1, "cols_P16": 1, "cols_P8": 2, "scalar_P63": 1, "scalar_P2": 2,
             "past_P65": 0, "past_P57": 0, "past_P9": 0, "past_P1": 0, "eight": 6}


@pytest.mark.parametrize("name,cfg", TAIL_CONFIGS, ids=[c[0] for c in TAIL_CONFIGS])
def test_whole_tail_in_its_four_forms(gpu, name, cfg):
    """Separate launches / a recorded chain phase by phase / fused / fused with the one-pass site code: bit-equal
    among themselves (parameters, both moments, the left-over gradient, d_value, the guide's parameter gradients,
    the total), the separate launches within the rule of the float64 reference per element, and the number of
    sites that took the one-pass form is what the restated eligibility rule predicts -- on both sides of
    P = 8 min(8, 256 / n), of n = 256 and of 2 <= P <= 64 for the scalar layout."""
    assert cfg["fast"] == TAIL_FAST[name]
    args = (cfg["sites"], cfg["inp"], cfg["P"], cfg["xcoef"], cfg["clipped"], cfg["zero_grad"])
    runs = {}
    for form in FORMS:
        runs[form], rec = _tail(form, *args, True, gpu)
        if form == "phases":
            assert rec.stats == (1, 3) and rec.fused == 0 and rec.fast_sites == 0, (rec.stats, rec.fused)
        elif form == "fused":
            assert rec.stats == (1, 3) and rec.fused == 1 and rec.fast_sites == 0, (rec.stats, rec.fused, rec.fast_sites)
        elif form == "fast":
            assert rec.stats == (1, 3) and rec.fused == 1, (rec.stats, rec.fused)
            assert rec.fast_sites == cfg["fast"], (rec.fast_sites, cfg["fast"])
    _score_tail("tail/" + ("clipped" if cfg["clipped"] else "adam"), runs["separate"], *args, True)
    ref = runs["separate"]
    for form in FORMS[1:]:
        got = runs[form]
        for w in ("total", "p", "m", "v", "left"):
            assert torch.equal(ref[w], got[w]), "%s: %s differs from the separate launches" % (form, w)
        for w in ("d_value", "d_guide", "eps"):
            for a, b in zip(ref[w], got[w]):
                assert torch.equal(a, b), "%s: %s differs from the separate launches" % (form, w)


@pytest.mark.parametrize("name,cfg", [TAIL_CONFIGS[0], TAIL_CONFIGS[3], TAIL_CONFIGS[10]],
                         ids=["cols_P64", "cols_P8", "eight"])
def test_whole_tail_separate_launches_in_float64(gpu, name, cfg):
    args = (cfg["sites"], cfg["inp"], cfg["P"], cfg["xcoef"], cfg["clipped"], False)
    got, _ = _tail("separate", *args, False, gpu)
    _score_tail("tail/" + ("clipped" if cfg["clipped"] else "adam"), got, *args, False)


def test_zz_measured_ratios():
    """Prints the largest error / bound per kernel, path and dtype of this process's run (the table of
    tests/multisite_edge_cases.py's docstring); PYRO_AMD_MULTISITE_EDGE_RATIOS names a file to write it to.  Every
    ratio is under 1."""
    table = mc.ratio_table()
    print("\nerror / bound, largest per path:\n" + table)
    path = os.environ.get("PYRO_AMD_MULTISITE_EDGE_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write(table + "\n")
    assert all(v < 1.0 for v in mc.RATIOS.values())
