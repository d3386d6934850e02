"""The tables of tests/nuts_edge_cases.py on the CPU: the runners and checks through tests/oracle_backend.py,
and the conditions the tables themselves have to meet -- asserted here, not assumed: the undecidable share
of every float32 parametrisation, a divergence at a later leaf, a non-finite energy, full depth in every
depth-limit case -- plus the find_step oracle pinned to the host search of hmc.py."""
import math

import numpy as np
import pytest

from oracle import integrator as o_int
from oracle import nuts as o_nuts
from oracle import philox
from tests import nuts_edge_cases as nc
from tests import oracle_backend as ob

CPU = "cpu"
DTYPES = [pytest.param(True, id="f32"), pytest.param(False, id="f64")]


def _d_params():
    return [pytest.param(D, f32, id="D%d-%s" % (D, "f32-dpad%d" % nc.dpad_of(D) if f32 else "f64"))
            for f32 in (True, False) for D in (nc.D_EDGES_F32 if f32 else nc.D_EDGES_F64)]


@pytest.mark.parametrize("D,f32", _d_params())
def test_d_edges(D, f32):
    nc.check_rows(ob, CPU, nc.d_edge_rows(D, f32))


@pytest.mark.parametrize("f32", DTYPES)
def test_c_edges(f32):
    nc.check_rows(ob, CPU, nc.c_edge_rows(f32))


@pytest.mark.parametrize("f32", DTYPES)
def test_depth_limits_run_to_full_depth(f32):
    rows = nc.depth_limit_rows(f32)
    nc.check_rows(ob, CPU, rows)
    for row in rows:
        for o, _ in nc.reference(row).values():
            assert o["depth"] == row.depth and o["n_leapfrog"] == (1 << row.depth) - 1, row
            assert not o["diverging"]


def test_depth_10_fills_the_stack():
    nc.check_rows(ob, CPU, nc.DEPTH10_ROWS)
    for row in nc.DEPTH10_ROWS:
        assert row.depth == nc.NUTS_MAX_DEPTH
        for o, _ in nc.reference(row).values():
            assert o["depth"] == 10 and o["n_leapfrog"] == 1023, row


@pytest.mark.parametrize("f32", DTYPES)
def test_divergence_tables(f32):
    """Through both entry points; the tables hold a divergence at a later leaf, chains that do not diverge
    next to chains that do, first-leaf divergences in every chain and NaN energies."""
    rows = nc.divergence_rows(f32)
    nc.check_rows(ob, CPU, rows)
    nc.check_rows(ob, CPU, rows, through_run=True)
    late = calm = nan = 0
    for row in rows:
        outs = list(nc.reference(row).values())
        late += sum(o["diverging"] and o["n_leapfrog"] > 1 for o, _ in outs)
        calm += sum(not o["diverging"] for o, _ in outs)
        if row.steps == nc.FIRST_LEAF or row.steps in (nc.OVERFLOW32, nc.OVERFLOW64):
            assert all(o["diverging"] and o["n_leapfrog"] == 1 and not o["accepted"]
                       and o["accept_prob"] == 0.0 for o, _ in outs), row
        if row.steps in (nc.OVERFLOW32, nc.OVERFLOW64):
            # in the tensor dtype's own arithmetic the energy is not finite, and NaN in some chain
            for c in range(row.C):
                mg = nc.oracle_case(row, c, 0, nc.np_dtype(f32))[1]
                assert mg.nonfinite_energy == 1, (row, c)
                nan += mg.nan_energy
                assert mg.nan_energy <= (row.D > 1), (row, c)    # D = 1: inf, never inf - inf
    assert late >= 1 and calm >= 1 and nan >= 1


@pytest.mark.parametrize("f32", DTYPES)
def test_keys(f32):
    """chain_offset > 0 at the top of the transition index range: the draws are the oracle's with
    chain = offset + c (the backend and the reference both key them so), and differ from offset 0."""
    rows = nc.key_rows(f32)
    nc.check_rows(ob, CPU, rows)
    row = rows[0]
    moved = nc.oracle_case(row._replace(chain_offset=0), 0, nc.T_TOP)[0]
    assert not np.array_equal(moved["z"], nc.reference(row)[(nc.T_TOP, 0)][0]["z"])
    assert ((nc.T_TOP + 1) << 20) + 4096 < 1 << 64


def test_every_instantiation_is_reached():
    assert {nc.dpad_of(D) for D in nc.D_EDGES_F32} == set(nc.DPADS)
    for lo, hi in zip(nc.DPADS, nc.DPADS[1:]):          # both sides of every step of the ladder
        assert lo in nc.D_EDGES_F32 and lo + 1 in nc.D_EDGES_F32 and nc.dpad_of(lo + 1) == hi


def test_f32_tolerance_is_the_measured_one():
    """F32_DEV is the deviation of the numpy-float32 oracle from the float64 oracle on the committed
    tables (re-measured here on the D-edge rows of three instantiations), the decidable cases of the
    float32 oracle never differ in an integer output, and the share stays inside the cap."""
    rows = [r for D in (33, 97, 128) for r in nc.d_edge_rows(D, True)]
    res = nc.measure_f32_oracle(rows)
    print(res)
    assert res["z"] <= nc.F32_DEV and res["pe"] <= nc.F32_TOL and res["accept_prob"] <= nc.F32_TOL
    assert res["differ_decidable"] == 0
    assert res["undecidable"] <= nc.CAP * res["cases"]
    assert nc.F32_TOL == 4 * nc.F32_DEV and all(m <= nc.F32_TOL for m in nc.F32_MARGINS.values())
    q = dict(res["quantities"], slice=res["quantities"]["diverge"])
    assert all(q[kind] <= nc.F32_QDEV[kind] for kind in ("draw", "turn", "slice")), q
    fs = nc.measure_f32_find_step()
    print(fs)
    assert fs["delta"] <= nc.F32_QDEV["find_step"] and fs["differ_decidable"] == 0


# ---- find_step -------------------------------------------------------------------------------------------
def _hmc_find_step(z, pe, grad, pg, inv_mass, step, normals, min_step, max_step, threshold):
    """HMC._find_reasonable_step_size (pyro_amd/infer/mcmc/hmc.py) for one chain in plain Python, its
    draws injected: the loop, the kinetic energy and the leapfrog of the host path, not the kernel's
    statements."""
    trials = [0]

    def trial(step):
        r_u = normals(trials[0])
        trials[0] += 1
        r = r_u / np.sqrt(inv_mass)
        e0 = 0.5 * r_u.dot(r_u) + pe
        _, r1, _, pe1 = o_int.single_step_verlet(z, r, pg, inv_mass, step, grad)
        r1_u = np.sqrt(inv_mass) * r1
        delta = (0.5 * r1_u.dot(r1_u) + pe1) - e0
        return 1 if threshold < -delta else -1

    direction = trial(step)
    scale = 2.0 ** direction
    active = True
    for _ in range(200):
        active = active and min_step < step < max_step
        if not active:
            break
        step = step * scale
        active = active and trial(step) == direction
    return min(max(step, min_step), max_step), trials[0]


@pytest.mark.parametrize("name", sorted(nc.FS_CASES))
def test_find_step_oracle_is_the_host_search(name):
    """oracle.nuts.find_step_gaussian (the kernel restated) gives the step and the trial count of the host
    search on the same draws, and every case does what its name says."""
    for D in nc.FS_D:
        Lam, z, pe, g, im, step, lo, hi = nc.fs_inputs(name, D, False)
        pg = o_int.gaussian_potential(Lam)
        for c, (s, n, _) in enumerate(nc.fs_reference(name, D, False)):
            def normals(it, c=c):
                return philox.normal(D, np.float64, nc.FS_SEED, (nc.FS_KEY + it) << 20, nc.FS_OFFSET + c)
            with np.errstate(all="ignore"):
                hs, hn = _hmc_find_step(z[c], pe[c], g[c], pg, im[c] if im.ndim == 2 else im, step[c],
                                        normals, lo, hi, nc.FS_THRESHOLD)
            assert (s, n) == (hs, hn), (name, D, c)
            assert n <= 201 and math.isfinite(s)
            if name == "up":
                assert s > 4 * step[c]
            elif name == "down":
                assert s < step[c] / 4
            elif name == "clamp_hi":
                assert s == hi and n > 1
            elif name == "clamp_lo":
                assert s == lo and n > 1
            elif name == "outside_lo":
                assert s == lo and n == 1
            elif name == "outside_hi":
                assert s == hi and n == 1
            elif name == "nan":
                assert s == lo and n in (13, 14)    # about 1.0 halved down to 2^-12


def test_find_step_stops_after_200_scalings():
    """With bounds that never bind and a potential so flat that every trial accepts, the search stops at
    its trial bound with a finite step: 201 trials, the start times 2^200."""
    D = 2
    s, n = o_nuts.find_step_gaussian(np.zeros(D), 0.0, np.zeros(D), 1e-300 * np.eye(D), np.ones(D), 1.0,
                                     1, 0, 0, 0.0, math.inf, nc.FS_THRESHOLD, np.float64)
    assert n == 201 and s == 2.0 ** 200


@pytest.mark.parametrize("f32", DTYPES)
def test_find_step_through_the_backend(f32):
    n = und = 0
    for name in sorted(nc.FS_CASES):
        for D in nc.FS_D:
            a, b = nc.fs_check(name, D, f32, nc.fs_run(ob, CPU, name, D, f32))
            n, und = n + a, und + b
    assert und <= nc.CAP * n, (und, n)


# ---- adaptation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_accepts", [True, False])
@pytest.mark.parametrize("D", sorted(nc.ADAPT_ROWS))
def test_adaptation_restatement_against_the_backend(D, count_accepts):
    """The numpy restatement of the case module against the torch one of the backend, from the nonzero
    starting state; the divergent chain's accept_prob is 0 in every transition."""
    nc.adapt_check(D, nc.adapt_run(ob, CPU, D, count_accepts), count_accepts)
    ref = nc.adapt_reference(D)
    assert ref["counters"][0].min() >= nc.ADAPT_K
    if D == 128:
        assert ref["div"][:, 1:].any() and not ref["div"][:, 1:].all()
