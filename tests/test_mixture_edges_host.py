"""CPU checks of tests/mixture_edge_cases.py: the float64 references against sums written out by hand on tiny cases,
oracle/mixture.py against the references under the rule, the restated launch plans against brute-force walks (every
row owned once, every record slot written once, the empty-chunk cases really empty), and the unscored caps of the
float32 comparison from the references alone."""
import math

import numpy as np
import pytest
import torch

from oracle import mixture as o_mix
from tests import mixture_edge_cases as mx

F32, F64 = torch.float32, torch.float64


# ---- the references, by hand ---------------------------------------------------------------------------------------
def _lse(ts):
    m = max(ts)
    if m == -math.inf:
        return -math.inf
    return m + math.log(sum(math.exp(t - m) for t in ts))


def _normal(x, mu, sg):
    z = (x - mu) / sg
    return -0.5 * z * z - math.log(sg) - 0.5 * math.log(2 * math.pi), z / sg, (z * z - 1) / sg


def _expo(x, lam, _):
    return math.log(lam) - lam * x, 1 / lam - x, 0.0


@pytest.mark.parametrize("dist_id,fn", [(mx.NORMAL, _normal), (mx.EXPONENTIAL, _expo)])
@pytest.mark.parametrize("rows", [False, True])
def test_reference_equals_the_sums_written_out(dist_id, fn, rows):
    K, N, D, B = 3, 4, 2, 2
    c = mx.geometry(dist_id, N, K, D, B, rows=rows, seed=5)
    a = c.a.copy()
    a[0, ..., 1] = -math.inf                                # (a switched-off component in set 0)
    c = c.modified(a=a)
    ref = c.ref(F64)
    p0 = np.broadcast_to(c.p0, (B, K, D))
    p1 = np.broadcast_to(c.p1 if c.p1 is not None else 1.0, (B, K, D))
    for b in range(B):
        S, R = 0.0, [0.0] * K
        g0, g1 = np.zeros((K, D)), np.zeros((K, D))
        for n in range(N):
            ab = a[b, n] if rows else a[b]
            parts = [[fn(c.x[n, d], p0[b, k, d], p1[b, k, d]) for d in range(D)] for k in range(K)]
            ts = [ab[k] + sum(p[0] for p in parts[k]) for k in range(K)]
            l = _lse(ts)
            S += l
            for k in range(K):
                r = 0.0 if ts[k] == -math.inf else math.exp(ts[k] - l)
                assert abs(r - ref["r"][b, n, k]) <= 1e-14
                R[k] += r
                for d in range(D):
                    g0[k, d] += r * parts[k][d][1]
                    g1[k, d] += r * parts[k][d][2]
        assert abs(S - ref["S"][b]) <= 1e-12 * abs(S)
        np.testing.assert_allclose(ref["R"][b], R, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref["g0"][b], g0, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(ref["g1"][b], g1, rtol=1e-11, atol=1e-13)
    assert (ref["R"][0, 1] == 0) and (ref["g0"][0, 1] == 0).all()


def test_mvn_reference_equals_the_sums_written_out():
    K, N, D, B = 2, 3, 2, 1
    c = mx.mvn_geometry(N, K, D, B, seed=3)
    ref = c.ref(F64)
    W, loc = np.broadcast_to(c.W, (B, K, D, D)), np.broadcast_to(c.loc, (B, K, D))
    S, R, m, G = 0.0, np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D))
    rows = []
    for n in range(N):
        ts, zs, ds = [], [], []
        for k in range(K):
            d = [c.x[n, 0] - loc[0, k, 0], c.x[n, 1] - loc[0, k, 1]]
            z = [W[0, k, 0, 0] * d[0], W[0, k, 1, 0] * d[0] + W[0, k, 1, 1] * d[1]]
            ts.append(c.a[0, k] + math.log(W[0, k, 0, 0]) + math.log(W[0, k, 1, 1]) - math.log(2 * math.pi)
                      - 0.5 * (z[0] ** 2 + z[1] ** 2))
            zs.append(z), ds.append(d)
        l = _lse(ts)
        S += l
        for k in range(K):
            r = math.exp(ts[k] - l)
            R[k] += r
            for i in range(D):
                m[k, i] += r * zs[k][i]
                for j in range(i + 1):
                    G[k, i, j] += r * zs[k][i] * ds[k][j]
        rows.append(l)
    assert abs(S - ref["S"][0]) <= 1e-12 * abs(S)
    np.testing.assert_allclose(ref["R"][0], R, rtol=1e-12)
    np.testing.assert_allclose(ref["m"][0], m, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(ref["G"][0], G, rtol=1e-11, atol=1e-13)


def test_reference_conventions_dead_and_nan_rows():
    c = mx.geometry(mx.NORMAL, 6, 3, 2, 2, seed=1)
    x = c.x.copy()
    x[2, 1] = math.inf
    dead = c.modified(x=x)
    rd, keep = dead.ref(F64), c.modified(x=np.delete(c.x, 2, 0)).ref(F64)
    assert (rd["S"] == -math.inf).all()
    for q in ("R", "g0", "g1"):
        np.testing.assert_allclose(rd[q], keep[q], rtol=1e-14, atol=1e-15)     # (the sums pair differently)
    p0 = np.broadcast_to(c.p0, (2, 3, 2)).copy()
    p0[1, 2, 0] = math.nan
    rn = c.modified(p0=p0).ref(F64)
    for q in ("S", "R", "g0", "g1"):
        assert np.isnan(rn[q][1]).all() and np.isfinite(rn[q][0]).all()
    # torch's LogNormal at 0 is -inf - log 0: a NaN row; Gamma(alpha > 1) at 0 is a dead one
    ln = mx.geometry(mx.LOG_NORMAL, 4, 3, 1, 1, seed=2)
    x0 = ln.x.copy()
    x0[1, 0] = 0.0
    assert np.isnan(ln.modified(x=x0).ref(F64)["S"]).all()
    ga = mx.geometry(mx.GAMMA, 4, 3, 1, 1, seed=2)
    x0 = ga.x.copy()
    x0[1, 0] = 0.0
    rg = ga.modified(x=x0, p0=ga.p0 + 1.0).ref(F64)
    assert (rg["S"] == -math.inf).all() and np.isfinite(rg["g0"]).all() and np.isfinite(rg["g1"]).all()


# ---- oracle/mixture.py under the rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("dist_id", mx.FAMILIES)
def test_oracle_scalar_leaf_agrees_with_the_reference(dist_id):
    for K, N in ((1, 5), (3, 37), (5, 64)):
        c = mx.geometry(dist_id, N, K, 1, 1, seed=11)
        S, da, d0, d1 = o_mix.mixture_fwd_bwd(dist_id, c.x[:, 0], c.a[0], c.p0[0, :, 0],
                                              None if c.p1 is None else c.p1[0, :, 0])
        out = dict(S=np.array([S]), R=da[None], g0=d0[None, :, None], g1=d1[None, :, None])
        mx.score_leaf("host/oracle scalar", c, out, F64, {})


def test_oracle_diag_leaf_agrees_with_the_reference():
    for K, N, D in ((1, 5, 1), (3, 37, 3), (5, 64, 8)):
        c = mx.geometry(mx.NORMAL, N, K, D, 1, seed=12)
        S, da, dl, dc = o_mix.mixture_diag_normal_fwd_bwd(c.x, c.a[0], c.p0[0], c.p1[0])
        mx.score_leaf("host/oracle diag", c, dict(S=np.array([S]), R=da[None], g0=dl[None], g1=dc[None]), F64, {})


# ---- the launch plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "rows", "diag", "rows_diag"])
def test_lane_plans_own_every_row_once(kind):
    per_cu = 4 if kind in ("scalar", "rows") else 2
    unroll = 1 if kind == "diag" else mx.MIX_U
    shapes = [(K, N, B) for K in mx.LANE_K for N in mx.lane_ns(K) for B in (1, 3)] + [mx.LANE_DEEP[kind] + (1,)]
    for K, N, B in shapes:
        plan = mx.lane_plan(N, K, B, mx.MI355X_CUS, per_cu)
        own = mx.lane_walk(N, K, plan["grid"], unroll)
        rows = sorted(r for v in own.values() for r in v)
        assert rows == list(range(N)), (kind, K, N, B)
        assert max(len(v) for v in own.values()) == plan["rows_per_lane"], (kind, K, N, B)
        assert all(wg < plan["grid"] and wave < 4 and slot < 64 // plan["KP"] for wg, wave, slot in own)
    # the seams the N grid is there for
    for K in mx.LANE_K:
        rb = mx.rb_of(K)
        grids = [mx.lane_plan(N, K, 1, mx.MI355X_CUS, per_cu)["grid"] for N in mx.lane_ns(K)]
        assert grids[0] == 1 and max(grids) >= 2, (K, grids)           # a second workgroup
        assert mx.lane_plan(4 * rb + 1, K, 1, mx.MI355X_CUS, per_cu)["rows_per_lane"] == 5     # a second unrolled pass
    K, N = mx.LANE_DEEP[kind]
    plan = mx.lane_plan(N, K, 1, mx.MI355X_CUS, per_cu)
    nparts = plan["grid"] * (1 if per_cu == 4 else mx.MIX_WAVES)
    segs = mx.partial_segments(nparts)
    assert nparts > 128 and any(e >= 1 and r >= 1 for _, _, e, r in segs), (nparts, segs)


def test_partial_segments_read_every_partial_once():
    for nparts in list(range(1, 40)) + [127, 128, 129, 133, 140, 1024, 2051]:
        seen = []
        for b0, b1, eights, rest in mx.partial_segments(nparts):
            seen += list(range(b0, b1))
            assert eights * 8 + rest == max(0, b1 - b0)
        assert seen == list(range(nparts)), nparts


def test_event_plan_and_thread_maps():
    for DB in (16, 64, 256):
        own = mx.event_pairs(DB)
        assert sorted(own) == [(k, d) for k in range(16) for d in range(DB)]
        assert all(len(v) == 1 for v in own.values())
    for dist_id in mx.FAMILIES:
        for K, D, N, B, _, _ in mx.EVENT_SEAMS + (mx.EVENT_WIDE,):
            for f32 in (True, False):
                p = mx.event_plan(dist_id, K, D, B, N, f32)
                rows = [r for r0, r1 in p["chunk_rows"] for r in range(r0, r1)]
                assert rows == list(range(N)) and p["rows_per"] % mx.EV_TR == 0
                assert p["DC"] == (16 if f32 else 8) // (2 if dist_id == mx.GAMMA else 1)
                # finalize: feature d reads slot (d // DB, d % DB): one reader per written slot of a live feature
                slots = {(d // p["DB"], d % p["DB"]) for d in range(D)}
                assert len(slots) == D and max(s[0] for s in slots) == p["ndb"] - 1
    ds = {D: mx.event_plan(mx.NORMAL, 2, D, 1, 257, True) for D in (16, 17, 64, 65, 256, 257, 1024)}
    assert [ds[D]["DB"] for D in sorted(ds)] == [16, 64, 64, 256, 256, 256, 256]
    assert [ds[D]["ndb"] for D in sorted(ds)] == [1, 1, 1, 1, 1, 2, 4]
    # the empty trailing chunk
    K, D, N, B = mx.EVENT_EMPTY_CHUNK
    for f32 in (True, False):
        p = mx.event_plan(mx.NORMAL, K, D, B, N, f32)
        r0, r1 = p["chunk_rows"][-1]
        assert p["chunks"] == 4 and r0 >= N and r1 == N, p
        assert sum(max(0, b - a) for a, b in p["chunk_rows"]) == N


def test_mvn_plan_and_thread_maps():
    for DP in (8, 16, 32, 64):
        own = mx.mvn_blocks(DP)
        NB = DP // (DP // 16 if DP >= 16 else 1)
        assert sorted(own) == [(i, j) for i in range(NB) for j in range(i + 1)], DP
        assert all(len(v) == 1 for v in own.values())
        assert len(own) + DP + 1 <= mx.MVN_THREADS
    for D, K, N, B, _, _ in mx.MVN_SEAMS:
        for f32 in (True, False):
            p = mx.mvn_plan(K, D, B, N, f32)
            rows = [r for r0, r1 in p["chunk_rows"] for r in range(r0, r1)]
            assert rows == list(range(N)) and p["rows_per"] % p["TR"] == 0
    assert mx.mvn_plan(3, 64, 1, 257, False)["TR"] == 128 and mx.mvn_plan(3, 64, 1, 257, True)["TR"] == 256
    assert sorted({mx.mvn_plan(K, D, 1, 9, True)["TB"] for D, K, _, _, _, _ in mx.MVN_SEAMS}) == [1, 2, 4]
    K, D, N, B = mx.MVN_EMPTY_CHUNK
    p = mx.mvn_plan(K, D, B, N, True)
    r0, r1 = p["chunk_rows"][-1]
    assert p["chunks"] == 4 and p["rows_per"] == 512 and r0 >= N and r1 == N, p


# ---- the unscored caps ------------------------------------------------------------------------------------------------
def _unscored(case, outs):
    r64, r3 = case.ref(F64), case.ref(F32)
    return {q: (mx.unscored(r64[q], r3[q]), r64[q].size) for q in outs}


@pytest.mark.parametrize("dist_id", mx.FAMILIES)
def test_geometry_grids_leave_nothing_unscored(dist_id):
    outs = ("S", "R", "r", "g0", "g1")
    for args in ((257, 17, 1, 1), (65, 5, 3, 3), (257, 17, 17, 1)):
        for rows in (False, True):
            c = mx.geometry(dist_id, *args, rows=rows)
            assert all(n == 0 for n, _ in _unscored(c, outs).values()), (dist_id, args)
            assert all(np.isfinite(c.ref(F64)[q]).all() for q in outs)


def test_mvn_geometry_grids_leave_nothing_unscored():
    for D, K, N, B, sl, sw in mx.MVN_SEAMS[:8]:
        c = mx.mvn_geometry(N, K, D, B, sl, sw)
        r64, r3 = c.ref(F64), c.ref(F32)
        for q in ("S", "R", "m", "G"):
            assert mx.unscored(r64[q], r3[q]) == 0 and np.isfinite(r64[q]).all(), (D, K, N, q)


@pytest.mark.parametrize("dist_id", mx.FAMILIES)
def test_edge_grids_stay_within_the_unscored_cap(dist_id):
    for K, D, rows in mx.EDGE_SHAPES:
        c = mx.edge_case(dist_id, K, D, rows)
        assert c.N >= 8, (dist_id, K, D, c.N)
        for q, (n, size) in _unscored(c, ("S", "R", "r", "g0", "g1")).items():
            assert n <= mx.UNSCORED_CAP * size, (dist_id, K, D, q, n, size)


def test_parent_bits_cover_every_fixed_kernel_in_both_dtypes():
    keys = {"%s %s" % (name, dt) for name in mx.bits_cases() for dt in ("f32", "f64")}
    assert set(mx.PARENT_BITS) == keys
