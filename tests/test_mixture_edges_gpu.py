"""The six mixture leaves on the device, per output entry against the float64 references of
tests/mixture_edge_cases.py: every lane layout and launch-plan seam on ordinary data (A-C), exact integer cases that pin
which (k, d) owns which output slot (D), the non-finite conventions (E) and the measured error / bound ratios (F).
Every call runs twice and the two runs must agree bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests import mixture_edge_cases as mx

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]
LANE_KINDS = ("scalar", "rows", "diag", "rows_diag")
_ids = {"ids": lambda v: mx.dname(v) if isinstance(v, torch.dtype) else None}


def _cus():
    from pyro_amd import kernels
    return int(kernels._lib.load().pa_device_cu_count())


def _run(kind, case, dtype, gpu, **kw):
    """The leaf twice (bit-identical), its outputs as numpy float64."""
    o1 = mx.run_leaf(kind, case, dtype, gpu, **kw)
    o2 = mx.run_leaf(kind, case, dtype, gpu, **kw)
    assert mx.same_bits(o1, o2), "%s %s: two runs differ" % (kind, case.name)
    return o1


def _check(kind, case, dtype, gpu, label=None, **kw):
    out = _run(kind, case, dtype, gpu, **kw)
    label = "%s %s%s" % (kind, mx.dname(dtype), "" if label is None else " " + label)
    if kind == "mvn":
        mx.score_mvn(label, case, out, dtype, mx.leaf_ks(kind, case, dtype, _cus()))
    else:
        mx.score_leaf(label, case, out, dtype, mx.leaf_ks(kind, case, dtype, _cus()))
    return out


# ---- A. the lane layouts ---------------------------------------------------------------------------------------------
SHARES = (("", ""), ("k", ""), ("", "k"), ("b", "b"), ("", "b"), ("kb", ""))


def _lane_case(kind, dist_id, K, N, i):
    """The i-th shape of a kernel's geometry walk: B, D, the sharing and the layout of a rotate with i."""
    B = (1, 3)[i % 2]
    rows = kind in ("rows", "rows_diag")
    D = mx.DIAG_D[(i + K) % len(mx.DIAG_D)] if kind in ("diag", "rows_diag") else 1
    s0, s1 = SHARES[(i + K) % len(SHARES)]
    if kind in ("diag", "rows_diag"):
        s0, s1 = s0 + ("d" if i % 3 == 1 else ""), s1 + ("d" if i % 3 == 2 else "")
    layout = mx.ROW_LAYOUTS[(i + K) % 4] if rows else "rows"
    case = mx.geometry(dist_id, N, K, D, B, rows=rows, share0=s0, share1=s1, share_a=layout == "shared", seed=i)
    return case, (dict(layout=layout, want_da=(i + K) % 3 != 0) if rows else {})


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("K", mx.LANE_K)
@pytest.mark.parametrize("kind", LANE_KINDS)
def test_lane_layouts_over_the_geometry(gpu, kind, K, dtype):
    fams = (mx.NORMAL, mx.GAMMA) if kind in ("scalar", "rows") else (mx.NORMAL,)
    for dist_id in fams:
        for i, N in enumerate(mx.lane_ns(K)):
            case, kw = _lane_case(kind, dist_id, K, N, i)
            _check(kind, case, dtype, gpu, **kw)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", LANE_KINDS)
def test_lane_layouts_second_launch_past_its_eight_deep_loop(gpu, kind, dtype):
    K, N = mx.LANE_DEEP[kind]
    plan = mx.lane_plan(N, K, 1, _cus(), 4 if kind in ("scalar", "rows") else 2)
    nparts = plan["grid"] * (1 if kind in ("scalar", "rows") else mx.MIX_WAVES)
    assert any(e >= 1 and r >= 1 for _, _, e, r in mx.partial_segments(nparts)), nparts
    rows = kind in ("rows", "rows_diag")
    case = mx.geometry(mx.NORMAL, N, K, 1 if kind in ("scalar", "rows") else 5, 1, rows=rows, seed=3)
    _check(kind, case, dtype, gpu)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("dist_id", mx.FAMILIES)
@pytest.mark.parametrize("kind", ("scalar", "rows"))
def test_lane_layouts_every_family(gpu, kind, dist_id, dtype):
    for K, N, B in ((5, 257, 3), (17, 65, 1)):
        _check(kind, mx.geometry(dist_id, N, K, 1, B, rows=kind == "rows", seed=4), dtype, gpu, "families")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("dist_id", mx.FAMILIES)
def test_edge_grids(gpu, dist_id, dtype):
    for K, D, rows in mx.EDGE_SHAPES:
        case = mx.edge_case(dist_id, K, D, rows)
        kinds = (["rows" if rows else "scalar"] if D == 1 else []) + ([] if rows else ["event"])
        if dist_id == mx.NORMAL and D > 1:
            kinds.append("rows_diag" if rows else "diag")
        for kind in kinds:
            _check(kind, case, dtype, gpu, "edge")


# ---- B. the event leaf's seams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("seam", range(len(mx.EVENT_SEAMS)))
def test_event_seams(gpu, seam, dtype):
    K, D, N, B, s0, s1 = mx.EVENT_SEAMS[seam]
    for dist_id in (mx.NORMAL, mx.GAMMA, mx.BERNOULLI):
        _check("event", mx.geometry(dist_id, N, K, D, B, share0=s0, share1=s1, seed=seam), dtype, gpu)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_event_widest(gpu, dtype):
    K, D, N, B, s0, s1 = mx.EVENT_WIDE
    _check("event", mx.geometry(mx.NORMAL, N, K, D, B, share0=s0, share1=s1), dtype, gpu)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("dist_id", mx.FAMILIES)
def test_event_every_family(gpu, dist_id, dtype):
    _check("event", mx.geometry(dist_id, 257, 17, 17, 1, seed=6), dtype, gpu, "families")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_event_empty_trailing_chunk(gpu, dtype):
    K, D, N, B = mx.EVENT_EMPTY_CHUNK
    p = mx.event_plan(mx.NORMAL, K, D, B, N, dtype == F32)
    assert p["chunk_rows"][-1][0] >= N
    _check("event", mx.geometry(mx.NORMAL, N, K, D, B, share1="b", seed=7), dtype, gpu, "empty chunk")


# ---- C. the full-covariance leaf's seams -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("seam", range(len(mx.MVN_SEAMS)))
def test_mvn_seams(gpu, seam, dtype):
    D, K, N, B, sl, sw = mx.MVN_SEAMS[seam]
    _check("mvn", mx.mvn_geometry(N, K, D, B, sl, sw, seed=seam), dtype, gpu)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_mvn_empty_trailing_chunk(gpu, dtype):
    K, D, N, B = mx.MVN_EMPTY_CHUNK
    assert mx.mvn_plan(K, D, B, N, dtype == F32)["chunk_rows"][-1][0] >= N
    _check("mvn", mx.mvn_geometry(N, K, D, B, seed=8), dtype, gpu, "empty chunk")


# ---- D. exact indexing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", mx.KINDS)
def test_exact_indexing(gpu, kind, dtype):
    shapes = {"scalar": ((5, 263, 1), (17, 1031, 1)), "rows": ((5, 263, 1), (17, 1031, 1)),
              "diag": ((5, 263, 3), (17, 300, 8), (33, 150, 5)), "rows_diag": ((5, 263, 3), (17, 300, 8), (33, 150, 7)),
              "event": ((5, 263, 3), (17, 300, 17), (33, 513, 65), (3, 257, 257)),
              "mvn": ((5, 263, 3), (17, 300, 9), (3, 513, 17), (3, 259, 33), (4, 131, 64))}[kind]
    for K, N, D in shapes:
        case, exp = mx.exact_case(N, K, D, B=2, rows=kind in ("rows", "rows_diag"))
        eq = lambda got, want, what: np.testing.assert_array_equal(      # noqa: E731
            got, np.broadcast_to(want, got.shape), err_msg="%s K=%d N=%d D=%d %s" % (kind, K, N, D, what))
        if kind == "mvn":
            case = mx.MvnCase(case.x, case.a, case.p0, np.eye(D)[None, None], "exact")
            out = _run(kind, case, dtype, gpu)
            eq(out["R"], exp["R"], "R"), eq(out["m"], exp["dloc"], "m"), eq(out["G"], exp["G"], "G")
            continue
        out = _run(kind, case, dtype, gpu)
        eq(out["g0"], exp["dloc"], "dloc"), eq(out["g1"], exp["dscale"], "dscale")
        if out["R"] is not None:
            eq(out["R"], exp["R"], "R")
        if out["r"] is not None:
            eq(out["r"], exp["r"], "r")


# ---- E. the non-finite conventions ------------------------------------------------------------------------------------
def _base(kind, K, D, dist_id=mx.NORMAL, N=37, B=3):
    """An ordinary case of ``kind``: three sets, so that one can be hurt and the others must stay as they are."""
    if kind == "mvn":
        return mx.mvn_geometry(N, K, D, B, seed=30 + K, dense=True)
    return mx.geometry(dist_id, N, K, D, B, rows=kind in ("rows", "rows_diag"), seed=30 + K)


def _dims(kind):
    """D equal to and below the padded feature count."""
    return {"scalar": (1,), "rows": (1,), "diag": (3, 4), "rows_diag": (3, 4), "event": (7, 16), "mvn": (7, 8)}[kind]


def _grads(kind):
    return ("m", "G") if kind == "mvn" else ("g0", "g1")


def _put(arr, idx, value, shape=None):
    arr = np.array(np.broadcast_to(arr, shape) if shape is not None else arr, dtype=np.float64)
    arr[idx] = value
    return arr


def _finite(out, names):
    return all(out.get(q) is None or np.isfinite(out[q]).all() for q in names)


ALL = [(kind, K) for kind in mx.KINDS for K in (3, 5)]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,K", ALL)
def test_a_switched_off_component_gets_exact_zeros(gpu, kind, K, dtype):
    for D in _dims(kind):
        base = _base(kind, K, D)
        for k in range(K):
            idx = (1, slice(None), k) if base.a.ndim == 3 else (1, k)
            case = base.modified("component %d off" % k, a=_put(base.a, idx, -math.inf))
            out = _check(kind, case, dtype, gpu, "non-finite")
            if out["R"] is not None:
                assert out["R"][1, k] == 0
            if out.get("r") is not None:
                assert (out["r"][1, :, k] == 0).all()
            for q in _grads(kind):
                assert (out[q][1, k] == 0).all(), (kind, K, D, k, q, out[q][1, k])


def _dead_rows(kind, K, D):
    """(case, sets whose S must be -inf): an infinite first / last feature; x = 0 under Gamma(alpha > 1)."""
    base = _base(kind, K, D)
    for d in sorted({0, D - 1}):
        yield base.modified("row 5 dead by feature %d" % d, x=_put(base.x, (5, d), math.inf))
        yield base.modified("rows 0, 36 dead by feature %d" % d,
                            x=_put(_put(base.x, (0, d), -math.inf), (36, d), math.inf))
    if kind in ("scalar", "rows", "event"):
        g = _base(kind, K, D, mx.GAMMA)
        yield g.modified("Gamma row at 0", x=_put(g.x, (7, D - 1), 0.0), p0=g.p0 + 1.0)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,K", ALL)
def test_a_dead_row_adds_nothing(gpu, kind, K, dtype):
    for D in _dims(kind):
        for case in _dead_rows(kind, K, D):
            out = _check(kind, case, dtype, gpu, "non-finite")
            assert (out["S"] == -math.inf).all(), (case.name, out["S"])
            assert _finite(out, ("R", "r") + _grads(kind)), case.name


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", ("scalar", "rows", "event"))
def test_lognormal_at_zero_is_a_nan_row_as_in_torch(gpu, kind, dtype):
    """torch's LogNormal.log_prob(0) is -inf - log 0 = NaN: the reference has a NaN row there, not a dead one."""
    D = 1 if kind != "event" else 5
    base = _base(kind, 3, D, mx.LOG_NORMAL)
    case = base.modified("LogNormal row at 0", x=_put(base.x, (7, D - 1), 0.0))
    out = _check(kind, case, dtype, gpu, "non-finite")
    for q in ("S", "R", "g0", "g1"):
        assert out[q] is None or np.isnan(out[q]).all(), (q, out[q])


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,K", ALL)
def test_a_collapsed_component_keeps_its_gradients_finite(gpu, kind, K, dtype):
    """A live row with one component whose z^2 overflows float32 (scale 1e-20, offset about 1)."""
    for D in _dims(kind):
        base = _base(kind, K, D)
        for k in range(K):
            if kind == "mvn":
                W = np.array(np.broadcast_to(base.W, (base.B, K, D, D)))
                W[1, k][np.diag_indices(D)] = 1e20
                case = base.modified("component %d collapsed" % k, W=W)
            else:
                case = base.modified("component %d collapsed" % k,
                                     p1=_put(base.p1, (1, k), 1e-20, (base.B, K, D)))
            out = _check(kind, case, dtype, gpu, "non-finite")
            assert np.isfinite(out["S"]).all() and _finite(out, ("R", "r") + _grads(kind)), (kind, K, D, k)
            for q in _grads(kind):
                assert (out[q][1, k] == 0).all(), (kind, K, D, k, q)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,K", ALL)
def test_a_nan_data_row_makes_every_sum_nan(gpu, kind, K, dtype):
    for D in _dims(kind):
        base = _base(kind, K, D)
        for d in sorted({0, D - 1}):
            case = base.modified("NaN in row 11 feature %d" % d, x=_put(base.x, (11, d), math.nan))
            out = _check(kind, case, dtype, gpu, "non-finite")
            for q in ("S", "R") + _grads(kind):
                if out[q] is None:
                    continue
                got = out[q][..., np.tril(np.ones((D, D), bool))] if q == "G" else out[q]
                assert np.isnan(got).all(), (kind, K, D, d, q, got)
            if out.get("r") is not None:
                assert np.isnan(out["r"][:, 11]).all() and np.isfinite(np.delete(out["r"], 11, 1)).all()
            if kind == "mvn":
                up = np.triu(np.ones((D, D), bool), 1)
                assert (out["G"][..., up] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,K", ALL)
def test_a_nan_parameter_makes_its_set_nan_whatever_the_component(gpu, kind, K, dtype):
    for D in _dims(kind):
        base = _base(kind, K, D)
        for k in range(K):
            if kind == "mvn":
                case = base.modified("NaN loc of component %d" % k,
                                     loc=_put(base.loc, (1, k, D - 1), math.nan, (base.B, K, D)))
            else:
                case = base.modified("NaN p0 of component %d" % k,
                                     p0=_put(base.p0, (1, k, D - 1), math.nan, (base.B, K, D)))
            out = _check(kind, case, dtype, gpu, "non-finite")
            for q in ("S", "R") + _grads(kind):
                if out[q] is None:
                    continue
                got = out[q][1][..., np.tril(np.ones((D, D), bool))] if q == "G" else out[q][1]
                assert np.isnan(got).all(), (kind, K, D, k, q, got)
                assert np.isfinite(out[q][0]).all() and np.isfinite(out[q][2]).all(), (kind, K, D, k, q)
            if out.get("r") is not None:
                assert np.isnan(out["r"][1]).all() and np.isfinite(out["r"][[0, 2]]).all()


# ---- the fixes change no finite result ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_fixed_kernels_keep_the_parents_bits(gpu, dtype):
    """One geometry case per fixed kernel, bit for bit as the parent commit computed it (mixture_edge_cases.PARENT_BITS)."""
    got = {}
    for name, case in mx.bits_cases().items():
        key = "%s %s" % (name, mx.dname(dtype))
        got[key] = mx.bits_digest(mx.run_leaf(name.split("/")[0], case, dtype, gpu))
        print("PARENT_BITS %r: %r," % (key, got[key]))
    assert got == {key: mx.PARENT_BITS.get(key) for key in got}


# ---- F. the measured constants -----------------------------------------------------------------------------------------
def test_zz_measured_constants(gpu):
    """Prints the largest error / bound per kernel, dtype and path; the table of mixture_edge_cases.py's docstring."""
    assert mx.RATIOS, "runs after the cases of this module"
    for label in sorted(mx.RATIOS):
        print("RATIO %-28s %.3f" % (label, mx.RATIOS[label]))
    assert all(v < 1.0 for v in mx.RATIOS.values()), mx.RATIOS
