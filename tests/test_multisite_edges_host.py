"""The numpy restatements the host suites and the golden makers rest on -- oracle_backend.multi_log_prob_sum /
_grad / _sum_grad, meanfield_normal_sample_bwd and adam_step -- against the float64 references and under the rule
of tests/multisite_edge_cases.py, on the CPU and over the grids the HIP kernels are tested on; the thread-map
restatement (tk, ng, k, path labels) against a brute-force walk of the kernels' loops; and that the float32
comparison formulas leave nothing of the geometry grids unscored."""
import numpy as np
import pytest
import torch

from tests import dist_edge_cases as ec
from tests import guide_edge_cases as gc
from tests import multisite_edge_cases as mc
from tests import oracle_backend as ob

F64 = torch.float64


def _np(xs):
    return tuple(None if x is None else x.double().numpy() for x in xs)


def _restated(label, ents, coef_all, g, total=True):
    """The restatement on one table (chunks of 16 as the wrapper launches them) under the rule, in float64."""
    for lo in range(0, len(ents), mc.MAX_ENTRIES):
        chunk = ents[lo:lo + mc.MAX_ENTRIES]
        case = mc.assembly_case(chunk, coef_all, g, False)
        grads = [_np(x) for x in ob.multi_log_prob_grad(torch.tensor(g, dtype=F64), chunk, coef_all, F64, None)]
        tot = float(ob.multi_log_prob_sum(chunk, coef_all, F64, None)) if total else None
        mc.score_assembly("host/" + label, case, False, tot, grads, path_labels=False)
        if g == 1.0:
            t2, g2 = ob.multi_log_prob_sum_grad(chunk, coef_all, F64, None)
            mc.score_assembly("host/" + label, case, False, float(t2), [_np(x) for x in g2], path_labels=False)


def _geometry_tables():
    for C in mc.THREAD_MAP_C:
        yield "map", mc.thread_map_table(C)
    for frame in mc.PATTERN_FRAMES:
        for tb in mc.pattern_tables(*frame):
            yield "patterns", tb
    for frame in mc.DEGENERATE_FRAMES:
        for tb in mc.pattern_tables(*frame, masked=False):
            yield "degenerate", tb
    yield "odd", mc.odd_entries_table()
    for n in mc.TOTAL_N:
        yield "total", mc.total_table(n)
    for members in (1, 2, 3):
        for i, frame in enumerate(mc.PATTERN_FRAMES):
            yield "chain", mc.chain_table(members, frame, (0.5, -2.0, None)[(members + i) % 3], seed=i)
    yield "chain", mc.two_chains_table()


def test_assembly_restatement_over_the_geometry_grids():
    for label, ents in _geometry_tables():
        _restated(label, ents, -0.25, 1.7)
        if label in ("chain", "total", "odd"):
            _restated(label, ents, 2.0, 1.0)


def test_every_entry_of_a_total_alone():
    """The restated total of a table is the sum of its entries' own totals."""
    for n in mc.TOTAL_N:
        ents = mc.total_table(n)
        parts = [float(ob.multi_log_prob_sum([e], -0.25, F64, None)) for e in ents]
        case = mc.assembly_case(ents, -0.25, 1.0, False)
        for e, got, M in zip(ents, parts, case["M"][2]):
            alone = mc.assembly_case([e], -0.25, 1.0, False)
            mc.score("host/total/alone", "entry", np.float64(got), alone["ref"][0], M, False)
        mc.score("host/total", "sum of parts", np.float64(sum(parts)), case["ref"][0], case["M"][0], False)


def test_nothing_in_the_geometry_grids_is_unscored():
    """Every float32 comparison value (the same torch formula in float32) of every geometry table is finite where
    the float64 reference is."""
    for label, ents in _geometry_tables():
        for lo in range(0, len(ents), mc.MAX_ENTRIES):
            case = mc.assembly_case(ents[lo:lo + mc.MAX_ENTRIES], -0.25, 1.7, True)
            assert np.isfinite(case["ref"][0]) and mc.unscored(case["ref"][0], case["cpu32"][0]) == 0
            for r, c in zip(case["ref"][1], case["cpu32"][1]):
                for x, y in zip(r, c):
                    assert (x is None) == (y is None)
                    if x is not None:
                        assert np.isfinite(x).all() and mc.unscored(x, y) == 0, label
    for n in mc.BWD_N:
        for P in mc.bwd_P(n):
            c = mc.bwd_case(n, P, (True, True, True), True)
            for x, y in zip(c["ref"], c["cpu32"]):
                assert np.isfinite(x).all() and mc.unscored(x, y) == 0


@pytest.mark.parametrize("dist", sorted(ec.NAMES))
def test_restatement_of_a_chain_at_the_family_edges(dist):
    """The restated chain head's d_value = the head's own gradient + the chained Normal member's, per element at
    the family's edge grid, non-finite pattern included."""
    rng = np.random.default_rng(50 + dist)
    c = mc.edge_chain_case(dist, False, rng)
    with np.errstate(all="ignore"):
        grads = ob.multi_log_prob_grad(torch.tensor(1.0, dtype=F64), c["entries"], 2.0, F64, None)
    for what, got, ref, M in zip(("d_value", "d_p0", "d_p1"), grads[0], c["ref"], c["M"]):
        if ref is not None:
            mc.score("host/edges", "%s %s" % (ec.NAMES[dist], what), got.numpy(), ref, M, False)


def test_thread_map_restatement_is_self_consistent():
    """grad_map / k_grad / sum_map / k_sum against a brute-force walk of the kernels' loops: every element has
    exactly one owner, the owner is the documented thread, and no thread adds more than k terms."""
    for C in mc.THREAD_MAP_C:
        tk, ng = mc.grad_map(C)
        assert tk == min(C, 256) and ng == min(8, 256 // tk) and tk * ng <= 256
        for R in mc.thread_map_rows(C) + [3 * 8 * ng + 2]:
            own = mc.thread_elements(R, C)
            assert (own >= 0).all()
            r, c = np.indices((R, C))
            assert np.array_equal(own, (r % ng) * tk + c % tk)
            per_col = max(np.bincount(own[:, j], minlength=256).max() for j in range(min(C, tk)))
            assert per_col == mc.k_grad(R, C, 1, "rowred") or R == 1
            assert np.bincount(own.ravel(), minlength=256).max() == (mc.k_grad(R, C, 1, "scalar") if R > 1 and C > 1
                                                                     else mc.cdiv(R, ng) * mc.cdiv(C, tk))
    for n in mc.TOTAL_N:
        for e in mc.total_table(n):
            own = mc.sum_elements(e["rows"], e["cols"], min(n, 16))
            assert (own >= 0).all()
            wpe = mc.sum_map(e["cols"], min(n, 16))[0]
            assert wpe == {1: 16, 2: 8, 3: 5, 4: 4, 5: 3, 8: 2, 9: 1, 16: 1}[min(n, 16)]
            assert np.bincount(own.ravel()).max() == mc.k_sum(e["rows"], e["cols"], min(n, 16))
    # the labels change exactly at the documented borders
    assert [mc.bwd_path(n, 16) for n in (255, 256, 4095, 4096)] == ["narrow", "tile256", "tile256", "wide64"]
    assert mc.bwd_path(4096, 15) == "tile256" and mc.bwd_map(4096, 16) == (64, 4) and mc.bwd_map(33, 5) == (33, 7)
    assert mc.pattern_of((1, 33), 1, 33) == "full" and mc.pattern_of((1, 1), 9, 1) == "rowred"
    assert mc.grad_path(0, "rowred") == "operand_rowred" and mc.grad_path(2, "scalar") == "combined_scalar"
    for (n, P) in mc.FAST_COLS_ELIGIBLE:
        assert mc.fast_site_expected(n, P)
    for (n, P) in mc.FAST_COLS_FALLBACK:
        assert not mc.fast_site_expected(n, P)
    assert [mc.fast_site_expected(1, P) for P in (1, 2, 63, 64, 65)] == [False, True, True, True, False]
    assert not mc.fast_site_expected(32, 64, prior=6) and not mc.fast_site_expected(32, 64, masked=True)


def _t(x):
    return None if x is None else torch.tensor(x, dtype=F64)


def test_backward_restatement_over_the_grid():
    """oracle_backend.meanfield_normal_sample_bwd: every n of the grid at two P, every None-combination, plain and
    into sinks holding 1.5."""
    for n in mc.BWD_N:
        for P in (mc.bwd_P(n)[1], 16):
            for which in mc.WHICH:
                c = mc.bwd_case(n, P, which, False)
                i = c["inp"]
                args = ([_t(i["rho"])], [_t(i["eps"])], [_t(i["d_z"]) if which[0] else None],
                        [_t(i["d_scale"]) if which[1] else None], [_t(i["d_loc_out"]) if which[2] else None], P)
                dl, dr = ob.meanfield_normal_sample_bwd(*args)
                mc.score_bwd("host/bwd", (dl[0].numpy(), dr[0].numpy()), c, False)
                sinks = [(torch.full((n,), 1.5, dtype=F64), torch.full((n,), 1.5, dtype=F64))]
                ob.meanfield_normal_sample_bwd(*args, sinks=sinks)
                mc.score_bwd("host/bwd/sinks", (sinks[0][0].numpy(), sinks[0][1].numpy()), c, False, add=1.5)


def _host_tail(sites, inp, P, coef_all, xcoef, clipped, zero_grad):
    """The tail through the restatements: draw, assembly, backward into the flat gradient, optimizer."""
    flat = {w: torch.tensor(inp[w], dtype=F64) for w in "pgmv"}
    locs = [flat["p"][o:o + n] for o, n in inp["locs"]]
    rhos = [flat["p"][o:o + n] for o, n in inp["rhos"]]
    zs, scales, louts, epss = ob.meanfield_normal_sample(locs, rhos, P, 11, [100 * k for k in range(len(sites))])
    ents = []
    for k, (s, z, sc, lo) in enumerate(zip(sites, zs, scales, louts)):
        n, prior, p0, p1, m = s
        fr = (1, P) if n == 1 else (P, n)
        ents.append(dict(dist=prior, rows=fr[0], cols=fr[1], value=z.reshape(fr), p0=p0, p1=p1, mask=m, coef=1.0,
                         need=(True, False, False), chain_next=2 * k + 1,
                         extra_grad=None if xcoef is None else torch.tensor(inp["extra"][k]).reshape(fr),
                         extra_coef=0.0 if xcoef is None else xcoef))
        ents.append(dict(dist=0, rows=fr[0], cols=fr[1], value=z.reshape(fr), p0=lo.reshape(1, n), p1=sc.reshape(1, n),
                         mask=None, coef=-1.0, need=(True, True, True), by_chain=True))
    total, grads = ob.multi_log_prob_sum_grad(ents, coef_all, F64, None)
    d_zs = [grads[2 * k][0].reshape(P, s[0]) for k, s in enumerate(sites)]
    sinks = [(flat["g"][o:o + n], flat["g"][o2:o2 + n]) for (o, n), (o2, _) in zip(inp["locs"], inp["rhos"])]
    ob.meanfield_normal_sample_bwd(rhos, epss, d_zs, [grads[2 * k + 1][2].reshape(-1) for k in range(len(sites))],
                                   [grads[2 * k + 1][1].reshape(-1) for k in range(len(sites))], P, sinks=sinks)
    grad = flat["g"].clone()
    hy = dict(mc.TAIL_HYPER) if clipped else dict(mc.TAIL_HYPER, clip=0.0, lrd=1.0)
    step = torch.tensor([mc.TAIL_STEP0, 0])
    ob.adam_step(flat["p"], flat["g"], flat["m"], flat["v"], step, lr=hy["lr"], betas=hy["betas"], eps=hy["eps"],
                 weight_decay=hy["wd"], clip_norm=hy["clip"], lrd=hy["lrd"], clipped=clipped, zero_grad=zero_grad)
    assert step.tolist() == [mc.TAIL_STEP0 + 1, 0]
    return dict(total=float(total), d_value=[x.numpy() for x in d_zs], grad=grad.numpy(), left=flat["g"].numpy(),
                p=flat["p"].numpy(), m=flat["m"].numpy(), v=flat["v"].numpy(), eps=[e.numpy() for e in epss])


@pytest.mark.parametrize("clipped", [False, True], ids=["adam", "clipped"])
def test_whole_tail_through_the_restatements(clipped):
    """Draw, assembly with chains and the extra term, backward into the flat gradient and the optimizer, restated,
    against autograd + torch.optim.Adam / the ClippedAdam formula: a mixed table (a scalar site of the n = 1
    frame [1, P], a Normal site, a masked head, a Gamma prior)."""
    P, shapes = 5, (1, 33, 4, 3)
    sites = mc.tail_sites(shapes, P, 1, priors=(0, 0, 0, 6), masked=(False, False, True, False))
    for xcoef in (None, 0.5):
        inp = mc.tail_inputs(sites, P, clipped, 1)
        got = _host_tail(sites, inp, P, -0.2, xcoef, clipped, zero_grad=xcoef is None)
        ref = mc.tail_reference(sites, inp, got["eps"], P, -0.2, xcoef, clipped, F64)
        M = mc.tail_magnitudes(sites, inp, got["eps"], P, -0.2, xcoef, ref, clipped)
        mc.score("host/tail", "total", np.float64(got["total"]), ref["total"], M["total"], False)
        for k in range(len(sites)):
            mc.score("host/tail", "d_value %d" % k, got["d_value"][k], ref["d_value"][k], M["d_value"][k], False)
        for w in ("grad", "p", "m", "v"):
            mc.score("host/tail", w, got[w], ref[w], M[w], False)
        assert np.array_equal(got["left"], np.zeros_like(got["left"]) if xcoef is None else got["grad"])


def test_tail_adam_reference_is_guide_edge_cases():
    """The tail's optimizer reference is the guide module's: torch.optim.Adam from a preset state."""
    c = gc.adam_case(False, 0, 1, 61, False)
    got = gc.torch_adam_step(c["p"], c["g"], c["m"], c["v"], 1, c["hy"], F64)
    for a, b in zip(got, c["ref"]):
        assert np.array_equal(a, b)
