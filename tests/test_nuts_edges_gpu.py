"""The fused Gaussian NUTS kernels of pyro_amd/csrc/nuts.hip tree for tree against oracle/nuts.py, in
float64 and in float32 (both float32 variants, every DPAD instantiation), at the edges of D, C, the tree
depth, divergence and the draw keys; pa_nuts_gaussian_find_step trial for trial; the in-kernel adaptation
of pa_nuts_gaussian_run against a numpy restatement.  Tables, runners and tolerances:
tests/nuts_edge_cases.py."""
import contextlib

import pytest
import torch

from tests import nuts_edge_cases as nc

pytestmark = pytest.mark.gpu

# float32 launch paths: the register kernel nuts_gaussian_reg_kernel<DPAD> (one wave per workgroup) and
# the LDS kernel nuts_gaussian_kernel<float, 4> (four waves per workgroup); float64 is always the LDS
# kernel nuts_gaussian_kernel<double, 2> (or <double, 1> when two waves' stacks do not fit: D = 128).
PATHS = [pytest.param(True, False, id="f32-reg"), pytest.param(True, True, id="f32-lds"),
         pytest.param(False, False, id="f64")]


def _k():
    from pyro_amd import kernels
    return kernels


@contextlib.contextmanager
def _variant(force_lds):
    from pyro_amd import _lib
    _lib.load().pa_nuts_gaussian_set_variant(int(force_lds))
    try:
        yield
    finally:
        _lib.load().pa_nuts_gaussian_set_variant(0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the largest error per quantity and the undecidable share of the module's run."""
    yield
    for key, st in sorted(_STATS.items()):
        print("\n%s: %s" % (key, {n: ("%.3g" % v if isinstance(v, float) else v) for n, v in st.items()}))


_STATS = {}


def _check(gpu, rows, f32, lds, **kw):
    st = _STATS.setdefault("f32-lds" if lds else "f32-reg" if f32 else "f64", {"cases": 0, "undecidable": 0})
    with _variant(lds):
        n, und = nc.check_rows(_k(), gpu, rows, stats=st, **kw)
    st["cases"] += n
    st["undecidable"] += und


def _d_params():
    out = []
    for D in nc.D_EDGES_F32:       # the id names the register-kernel instantiation the D selects
        out.append(pytest.param(D, True, False, id="D%d-f32-reg-dpad%d" % (D, nc.dpad_of(D))))
        out.append(pytest.param(D, True, True, id="D%d-f32-lds-wpb4" % D))
    for D in nc.D_EDGES_F64:
        out.append(pytest.param(D, False, False, id="D%d-f64-lds-wpb%d" % (D, 1 if D > 112 else 2)))
    return out


@pytest.mark.parametrize("D,f32,lds", _d_params())
def test_d_edges(gpu, D, f32, lds):
    """Both samplers, 12 chains, three transition indices per D; inv_mass per chain and dimension."""
    _check(gpu, nc.d_edge_rows(D, f32), f32, lds)


@pytest.mark.parametrize("f32,lds", PATHS)
def test_c_edges(gpu, f32, lds):
    """C = 1, 3, 5: the last workgroup of the LDS kernels has waves without a chain."""
    _check(gpu, nc.c_edge_rows(f32), f32, lds)


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_no_chains(gpu, f32):
    """C = 0 returns without a launch: empty outputs, nothing written."""
    k = _k()
    dt = torch.float32 if f32 else torch.float64
    D = 5
    e = lambda *s: torch.zeros(s, dtype=dt, device=gpu)         # noqa: E731
    L = torch.eye(D, dtype=dt, device=gpu)
    out = k.nuts_gaussian_transition(e(0, D), e(0), e(0, D), L, e(0, D), e(0), 5, True, 1, 0)
    assert all(v.shape == (0,) for v in out.values())
    counters = torch.zeros((3, 0), dtype=torch.int64, device=gpu)
    k.nuts_gaussian_run(e(0, D), e(0), e(0, D), L, e(0, D), e(0), 5, True, 1, 0, 4, counters=counters,
                        samples=e(4, 0, D))
    assert torch.equal(k.nuts_gaussian_find_step(e(0, D), e(0), e(0, D), L, e(0, D), e(0), 1, 0, 0, 1e-3,
                                                 1e3, -0.2), e(0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("f32,lds", PATHS)
def test_depth_limits(gpu, f32, lds):
    """max_tree_depth 1 and 3 with steps so small that every chain runs to the limit."""
    _check(gpu, nc.depth_limit_rows(f32), f32, lds)


def test_depth_10_fills_the_stack(gpu):
    """max_tree_depth = NUTS_MAX_DEPTH: 1023 leapfrogs per chain, every slot of the pending-subtree stack
    in use (float64; D = 65 multinomial, D = 128 slice)."""
    _check(gpu, nc.DEPTH10_ROWS, False, False)


@pytest.mark.parametrize("through_run", [False, True], ids=["transition", "run-div_flags"])
@pytest.mark.parametrize("f32,lds", PATHS)
def test_divergence(gpu, f32, lds, through_run):
    """Mixed, first-leaf and overflowing steps: a diverged, unaccepted chain comes back bit for bit, the
    NaN energy counts as +inf, accept_prob is the oracle's; through pa_nuts_gaussian_run the [1, C]
    div_flags and the counters carry the same."""
    _check(gpu, nc.divergence_rows(f32), f32, lds, through_run=through_run)


@pytest.mark.parametrize("f32,lds", PATHS)
def test_keys(gpu, f32, lds):
    """chain_offset > 0 and t = 2^43 - 2: the draws of chain offset + c at the top of the index range."""
    _check(gpu, nc.key_rows(f32), f32, lds)


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_refused_arguments(gpu, f32):
    """Argument checks of nuts_common_checks, all before any launch: t = 2^43, D = 129, max_tree_depth 0
    and 11, a find_step key of 2^43.  The state is not touched."""
    from pyro_amd import _lib
    k = _k()
    dt = torch.float32 if f32 else torch.float64

    def state(C, D):
        z = torch.ones((C, D), dtype=dt, device=gpu)
        return [z, torch.ones(C, dtype=dt, device=gpu), z.clone(), torch.eye(D, dtype=dt, device=gpu),
                z.clone(), torch.full((C,), 0.1, dtype=dt, device=gpu)]

    for D, depth, t, err in [(4, 5, 1 << 43, ValueError), (4, 5, (1 << 43) - 1, ValueError),
                             (129, 5, 0, _lib.Unsupported), (4, 0, 0, ValueError), (4, 11, 0, ValueError)]:
        st = state(3, D)
        with pytest.raises(err, match="nuts_gaussian"):
            k.nuts_gaussian_transition(*st, depth, True, 1, t)
        assert bool((st[0] == 1).all()) and bool((st[1] == 1).all())
    st = state(3, 4)
    with pytest.raises(ValueError, match="key too large"):
        k.nuts_gaussian_find_step(*st, 1, 1 << 43, 0, 1e-3, 1e3, -0.2)
    with pytest.raises(_lib.Unsupported):
        k.nuts_gaussian_find_step(*state(3, 129), 1, 0, 0, 1e-3, 1e3, -0.2)


# ---- find_step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("D", nc.FS_D)
def test_find_step_matches_the_restatement(gpu, D, f32):
    """Every case of FS_CASES, 8 chains each: the step equals the oracle's exactly (the start times a power
    of two, or a bound)."""
    n = und = 0
    for name in sorted(nc.FS_CASES):
        a, b = nc.fs_check(name, D, f32, nc.fs_run(_k(), gpu, name, D, f32))
        n, und = n + a, und + b
    assert und <= nc.CAP * n, (und, n)
    st = _STATS.setdefault("find_step-" + ("f32" if f32 else "f64"), {"cases": 0, "undecidable": 0})
    st["cases"] += n
    st["undecidable"] += und


# ---- adaptation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_accepts", [True, False], ids=["sampling", "warmup"])
@pytest.mark.parametrize("D", sorted(nc.ADAPT_ROWS))
def test_in_kernel_adaptation(gpu, D, count_accepts):
    """Six transitions in one launch from a nonzero adaptation state: step, da_state, welford, mean_accept,
    samples, counters and the [K, C] div_flags against the restatement driven by the oracle."""
    nc.adapt_check(D, nc.adapt_run(_k(), gpu, D, count_accepts), count_accepts)
