"""The kernels that end every SVI step -- pa_adam_step / _publish, pa_gamma_rsample / _implicit_grad,
pa_mvn_tril_sample / _bwd, pa_exp_site_fwd / _bwd and pa_meanfield_score -- per element against the float64
references and under the tolerance rule of tests/guide_edge_cases.py, at the sizes where their launch paths
change, with canaries around every buffer they write."""
import os

import numpy as np
import pytest
import torch

from tests import guide_edge_cases as gc

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(True, id="f32"), pytest.param(False, id="f64")]
BOTH = [pytest.param(False, id="adam"), pytest.param(True, id="clipped")]
PAD, FILL = 64, -777.25


def _k():
    from pyro_amd import kernels
    return kernels


def _cus():
    from pyro_amd import _lib
    return int(_lib.load().pa_device_cu_count())


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    """Prints the largest error / bound per kernel, path and dtype of the module's run (the table of
    tests/guide_edge_cases.py's docstring); PYRO_AMD_GUIDE_EDGE_RATIOS names a file to write it to."""
    yield
    table = gc.ratio_table() + "\n" + "\n".join("  %-28s %.3g" % kv for kv in sorted(GAMMA_REL.items()))
    print("\nerror / bound, largest per path:\n" + table)
    path = os.environ.get("PYRO_AMD_GUIDE_EDGE_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write(table + "\n")


GAMMA_REL = {}       # "gamma/grad/<branch>/<dtype> rel" -> largest relative error seen on the device


class Carved:
    """A buffer of n elements inside a larger allocation: PAD canary elements on either side."""

    def __init__(self, shape, f32, gpu, init=None, dtype=None):
        n = int(np.prod(shape))
        self.n = n
        dtype = dtype or gc.dt(f32)
        self.fill = FILL if dtype.is_floating_point else int(FILL)
        self.big = torch.full((n + 2 * PAD,), self.fill, dtype=dtype, device=gpu)
        self.t = self.big[PAD:PAD + n].view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(init).reshape(shape))

    def intact(self):
        return bool((self.big[:PAD] == self.fill).all() and (self.big[PAD + self.n:] == self.fill).all())


def _np(t):
    return t.detach().double().cpu().numpy()


# =======================================================================================================
# Adam / ClippedAdam
# =======================================================================================================

def _adam_launch(c, f32, gpu, zero_grad=True, chained=False, publish=None, lr=None):
    """One launch on carved buffers -> ((p, m, v) tensors, g tensor, step_dev list, chain stats)."""
    k = _k()
    hy = c["hy"]
    n = c["p"].size
    b = {w: Carved((n,), f32, gpu, c[w]) for w in "pgmv"}
    step = Carved((2,), f32, gpu, [c["step0"], 0], dtype=torch.int64)
    args = (b["p"].t, b["g"].t, b["m"].t, b["v"].t, step.t)
    kw = dict(lr=hy["lr"] if lr is None else lr, betas=hy["betas"], eps=hy["eps"], weight_decay=hy["wd"],
              clip_norm=hy["clip"], lrd=hy["lrd"], clipped=c["clipped"], zero_grad=zero_grad, publish=publish)
    stats = None
    if chained:
        with k.chain_recording(gpu) as rec:
            k.adam_step(*args, **kw)
        stats = rec.stats
    else:
        k.adam_step(*args, **kw)
    torch.cuda.synchronize()
    assert all(x.intact() for x in b.values()) and step.intact(), "a canary next to an Adam buffer was overwritten"
    return (b["p"].t, b["m"].t, b["v"].t), b["g"].t, step.t.tolist(), stats


def _adam_one(label, c, f32, gpu, zero_grad=True):
    """A case on the standalone launch -- the rule on parameter and both moments, the step counter, the
    gradient zeroed or untouched -- and, in float32, once more as a lone phase of a recorded chain: the
    recording turns the launch into ONE chain kernel of ONE phase (asserted through rec.stats: it is a
    different launch path, csrc/chain.hip's chain_kernel walking virtual workgroups), bit-equal."""
    got, g, step, _ = _adam_launch(c, f32, gpu, zero_grad)
    gc.adam_check(label, tuple(_np(x) for x in got), c, f32)
    assert step == [c["step0"] + 1, 0]
    g_in = torch.as_tensor(c["g"]).to(gc.dt(f32))
    if zero_grad:
        assert (g == 0).all() and not torch.signbit(g).any()
    else:
        assert g.cpu().view(torch.int32 if f32 else torch.int64).equal(g_in.view(torch.int32 if f32 else torch.int64))
    if f32:
        got2, g2, step2, stats = _adam_launch(c, f32, gpu, zero_grad, chained=True)
        assert stats == (1, 1), stats
        assert step2 == step and _bits_equal(g, g2)
        for x, y in zip(got, got2):
            assert _bits_equal(x, y), "%s: the chained phase differs from the standalone launch" % label
    return got


def _bits_equal(x, y):
    it = torch.int32 if x.dtype == torch.float32 else torch.int64
    return torch.equal(x.contiguous().view(it), y.contiguous().view(it))


def _label(clipped, what, f32):
    return "%s/%s/%s" % ("clipped" if clipped else "adam", what, gc.dname(f32))


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("clipped", BOTH)
def test_adam_hyper_parameters_and_preset_steps(gpu, clipped, f32):
    """Every hyper-parameter set (three beta pairs x eps 1e-8 / 1e-3 with gradients of order 1e-3 x weight decay
    x, for ClippedAdam, clip_norm 10 / 0.5 x lrd 1 / 0.99) from a given state with the step counter preset to
    0, 1, 999 or 100 000, n = 257 (two workgroups: the ticket)."""
    for i, (h, step0) in enumerate(gc.adam_single_keys(clipped)):
        _adam_one(_label(clipped, "single", f32), gc.adam_case(clipped, h, step0, 257, f32), f32, gpu,
                  zero_grad=i % 3 != 2)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("clipped", BOTH)
def test_adam_sizes(gpu, clipped, f32):
    """n = 1, 2, 255, 256 (one workgroup: no ticket), 257, 1000 and one n past 8 * CUs workgroups (threads
    loop); the default set at every preset step count for n <= 2, cycling above."""
    sizes = gc.ADAM_N + (gc.adam_grid_stride_n(_cus()),)
    for i, n in enumerate(sizes):
        for step0 in (gc.ADAM_STEP0 if n <= 2 else (gc.ADAM_STEP0[i % 4],)):
            path = "one_wg" if n <= 256 else "stride" if n > 8 * _cus() * 256 else "ticket"
            _adam_one(_label(clipped, path, f32), gc.adam_case(clipped, 0, step0, n, f32), f32, gpu)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("clipped", BOTH)
def test_adam_edge_gradients(gpu, clipped, f32):
    """All-zero gradients (with zero moments denom = eps and nothing moves), g = 1e25 (float32: g^2 overflows,
    the pattern is the CPU formula's), a NaN and an inf in one pool element each: every other element is
    bit-equal to the run without them."""
    label = _label(clipped, "edge", f32)
    got = _adam_one(label, gc.adam_case(clipped, 0, 1, 257, f32, "zero"), f32, gpu)
    assert _np(got[0]).tolist() == gc.adam_case(clipped, 0, 1, 257, f32, "zero")["p"].tolist()
    _adam_one(label, gc.adam_case(clipped, 0, 1, 257, f32, "zero_state"), f32, gpu)
    c = gc.adam_case(clipped, 0, 1, 257, f32, "big")      # (ClippedAdam clamps it to clip_norm = 10 first)
    got = _adam_one(label, c, f32, gpu)
    at = np.isin(np.arange(257) % gc.ADAM_POOL, gc.ADAM_BIG_AT)
    if f32 and not clipped:
        assert np.isinf(_np(got[2])[at]).all() and np.array_equal(_np(got[0])[at], c["p"][at])
    poisoned = _adam_one(label, gc.adam_case(clipped, 0, 1, 257, f32, "naninf"), f32, gpu)
    clean = _adam_one(label, gc.adam_case(clipped, 0, 1, 257, f32), f32, gpu)
    keep = torch.as_tensor(~np.isin(np.arange(257) % gc.ADAM_POOL, (gc.ADAM_NAN_AT, gc.ADAM_INF_AT)), device=gpu)
    for x, y in zip(poisoned, clean):
        assert _bits_equal(x[keep], y[keep])
    nan_at = np.arange(257) % gc.ADAM_POOL == gc.ADAM_NAN_AT
    assert all(np.isnan(_np(x)[nan_at]).all() for x in poisoned)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("clipped", BOTH)
def test_adam_zero_learning_rate(gpu, clipped, f32):
    """lr = 0 without weight decay: parameter and both moments bit-unchanged, the step advances, gradients
    zeroed on request only.  lr = 0 with weight decay: the moments move as the reference's do."""
    c = gc.adam_case(clipped, 0, 999, 257, f32)
    for zero in (True, False):
        got, g, step, _ = _adam_launch(c, f32, gpu, zero_grad=zero, lr=0.0)
        for x, w in zip(got, "pmv"):
            assert _bits_equal(x.cpu(), torch.as_tensor(c[w]).to(gc.dt(f32)))
        assert step == [1000, 0]
        assert (g == 0).all() if zero else _bits_equal(g.cpu(), torch.as_tensor(c["g"]).to(gc.dt(f32)))
    c = gc.adam_case(clipped, 0, 1, 257, f32, "lr0wd")
    got = _adam_one(_label(clipped, "lr0wd", f32), c, f32, gpu)
    assert not np.array_equal(_np(got[1]), c["m"]) and not np.array_equal(_np(got[2]), c["v"])
    assert np.array_equal(_np(got[0]), c["p"])


@pytest.mark.parametrize("clipped", BOTH)
def test_adam_trajectory(gpu, clipped):
    """Five steps in float64 from zero moments (weight decay, and for ClippedAdam an active clamp and lrd < 1):
    parameter and moments after every step under the rule, M from the reference's state before the step."""
    k = _k()
    p0, grads, want = gc.adam_trajectory(clipped)
    hy = gc.ADAM_TRAJ_HYPER
    n = 257
    tile = lambda x: np.resize(x, n)      # noqa: E731
    b = {w: Carved((n,), False, gpu, tile(x)) for w, x in zip("pmv", (p0, np.zeros_like(p0), np.zeros_like(p0)))}
    step = torch.zeros(2, dtype=torch.int64, device=gpu)
    p, m, v = (tile(x) for x in (p0, np.zeros_like(p0), np.zeros_like(p0)))
    for s, g in enumerate(grads):
        tg = Carved((n,), False, gpu, tile(g))
        k.adam_step(b["p"].t, tg.t, b["m"].t, b["v"].t, step, lr=hy["lr"], betas=hy["betas"], eps=hy["eps"],
                    weight_decay=hy["wd"], clip_norm=hy["clip"] if clipped else 0.0,
                    lrd=hy["lrd"] if clipped else 1.0, clipped=clipped)
        assert step.tolist() == [s + 1, 0] and tg.intact() and (tg.t == 0).all()
        M = gc.adam_magnitudes(p, tile(g), m, v, s, hy, clipped, tile(want[s][2]))
        p, m, v = (tile(x) for x in want[s])
        for what, w, ref, Mx in zip(("param", "exp_avg", "exp_avg_sq"), "pmv", (p, m, v), M):
            gc.check(_label(clipped, "traj", False), what, _np(b[w].t), ref, Mx, False)
    assert all(x.intact() for x in b.values())


def test_adam_empty_buffer_only_bumps_the_counter(gpu):
    k = _k()
    for dtype in (torch.float32, torch.float64):
        e = [torch.empty(0, dtype=dtype, device=gpu) for _ in range(4)]
        step = Carved((2,), True, gpu, [41, 0], dtype=torch.int64)
        k.adam_step(*e, step.t, lr=0.01)
        torch.cuda.synchronize()
        assert step.t.tolist() == [42, 0] and step.intact()


@pytest.mark.parametrize("n", [1, 257])
def test_adam_publish_at_one_element_and_across_the_ticket(gpu, n):
    """pa_adam_step_publish at n = 1 (one workgroup, no ticket) and n = 257 (the last arrival publishes): the
    update is bit-equal to the plain launch, sequence and counter advance once per launch."""
    c = gc.adam_case(True, 7, gc.adam_step0_of(True, 7), n, True)
    hv = torch.zeros(1, dtype=torch.float64).pin_memory()
    hs = torch.zeros(1, dtype=torch.int64).pin_memory()
    counter = torch.tensor([40, 100], dtype=torch.int64, device=gpu)
    loss = torch.full((), 2.5, device=gpu, dtype=torch.float32)
    plain, _, step_a, _ = _adam_launch(c, True, gpu)
    pub, g, step_b, _ = _adam_launch(c, True, gpu, publish=(loss, hv, hs, counter, 7))
    assert step_a == step_b == [c["step0"] + 1, 0] and (g == 0).all()
    for x, y in zip(plain, pub):
        assert _bits_equal(x, y)
    assert hs.item() == 101 and hv.item() == 2.5 and counter.tolist() == [47, 101]
    _adam_launch(c, True, gpu, publish=(loss, hv, hs, counter, 7))
    assert hs.item() == 102 and counter.tolist() == [54, 102]


# =======================================================================================================
# Gamma
# =======================================================================================================

@pytest.mark.parametrize("f32", DTYPES)
def test_gamma_implicit_gradient_on_the_fixture(gpu, f32):
    """pa_gamma_implicit_grad on the 60-digit grid: both sides of x = a + 1, of a = 1e4, of 8 standard
    deviations and of a = 1e8, a from 1e-3 to 3e8, the clamp values.  Relative bound per branch: 4 x the host
    oracle's measured maximum (at most 1e-9), plus one float32 rounding for the float32 instantiation (which
    stops its series at 1e-10)."""
    k = _k()
    a, x, ref = gc.gamma_grad_fixture(f32)
    ta, tx = Carved(a.shape, f32, gpu, a), Carved(x.shape, f32, gpu, x)
    got = _np(k.gamma_implicit_grad(ta.t, tx.t))
    assert np.array_equal(_np(ta.t), a) and np.array_equal(_np(tx.t), x)      # (the grid survives the dtype)
    ratios = gc.gamma_grad_ratios(got, a, x, ref, f32)
    br = gc.gamma_branch(a, x)
    for b, r in ratios.items():
        key = "gamma/grad/%s/%s" % (b, gc.dname(f32))
        gc.RATIOS[key] = max(gc.RATIOS.get(key, 0.0), r)
        big = (br == b) & (np.abs(ref) > (1e-30 if f32 else 1e-290))
        GAMMA_REL[key + " rel"] = float((np.abs(got - ref) / np.abs(ref))[big].max())
    print("\n", gc.dname(f32), "err / bound per branch:", ratios, {k_: v for k_, v in GAMMA_REL.items()})
    bad = np.flatnonzero(~(np.abs(got - ref) <= gc.gamma_grad_bound(a, x, ref, f32)))
    assert bad.size == 0, "\n".join("a=%.17g x=%.17g got %.17g ref %.17g (%s)" % (a[i], x[i], got[i], ref[i], br[i])
                                    for i in bad[:10])


@pytest.mark.parametrize("f32", DTYPES)
def test_gamma_implicit_gradient_of_an_infinite_argument_is_nan(gpu, f32):
    """x = inf or a = inf: NaN (the kernel returns at once instead of spending its iteration budget); a NaN
    argument gives 0 as every argument that is not > 0 does."""
    k = _k()
    d = gc.dt(f32)
    inf, nan = float("inf"), float("nan")
    a = torch.tensor([3.0, 3e8, inf, inf, nan, 3.0], dtype=d, device=gpu)
    x = torch.tensor([inf, inf, 5.0, inf, 1.0, nan], dtype=d, device=gpu)
    got = k.gamma_implicit_grad(a, x).cpu()
    assert torch.isnan(got[:4]).all() and got[4:].tolist() == [0.0, 0.0]


def _oracle_draws(alpha, seed, offset, f32):
    from oracle import gamma as o_gamma
    tiny = float(np.finfo(np.float32 if f32 else np.float64).tiny)
    return np.maximum(o_gamma.standard_gamma(alpha, seed, offset), tiny)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("shape", ["1x1", "3x85", "stride"])
def test_gamma_draws(gpu, f32, shape):
    """pa_gamma_rsample at 1 x 1, 3 x 85 and one launch past 8 * CUs workgroups: the draws are the oracle's
    (1e-12 / 5e-7, every element of every launch), a device-side offset adds to the host's,
    a stride-0 concentration reads the same blocks, the grid-stride tail equals a small launch whose offset is
    moved by the same count, float32 draws stop at 2^-126, and d_alpha is pa_gamma_implicit_grad at the
    returned values bit for bit."""
    k = _k()
    rows, cols = {"1x1": (1, 1), "3x85": (3, 85), "stride": (1, gc.adam_grid_stride_n(_cus()))}[shape]
    n = rows * cols
    alpha = gc.gamma_draw_alpha(rows, cols, f32)
    ta = torch.as_tensor(alpha, device=gpu).to(gc.dt(f32))
    seed, off = 42, 1234
    out, dal = k.gamma_rsample(ta, rows, cols, seed, off)
    tol = 5e-7 if f32 else 1e-12
    np.testing.assert_allclose(_np(out).reshape(-1), _oracle_draws(alpha.reshape(-1), seed, off, f32), rtol=tol)
    assert bool((out > 0).all()) and float(out.min()) >= float(np.finfo(np.float32 if f32 else np.float64).tiny)
    if f32 and shape == "stride":
        assert float(out.min()) == 2.0 ** -126        # (a = 0.05 puts 1.2 % of its mass below the clamp)
    # the gradient of the draws
    assert _bits_equal(dal, k.gamma_implicit_grad(ta, out))
    assert _bits_equal(out, k.gamma_rsample(ta, rows, cols, seed, off, want_grad=False)[0])
    # device-side offset
    off_dev = torch.tensor([1000], dtype=torch.int64, device=gpu)
    o2, d2 = k.gamma_rsample(ta, rows, cols, seed, off - 1000, off_dev)
    assert _bits_equal(out, o2) and _bits_equal(dal, d2)
    # the tail of the launch == a small launch moved by the same count
    t = min(n, 257)
    o3, d3 = k.gamma_rsample(ta.reshape(1, -1)[:, n - t:].contiguous(), 1, t, seed, off + n - t)
    assert _bits_equal(out.reshape(-1)[n - t:], o3.reshape(-1)) and _bits_equal(dal.reshape(-1)[n - t:], d3.reshape(-1))
    # stride-0 broadcast of one row / one element
    row = ta[:1]
    o4, _ = k.gamma_rsample(row, rows, cols, seed, off)
    o5, _ = k.gamma_rsample(row.expand(rows, cols).contiguous(), rows, cols, seed, off)
    assert _bits_equal(o4, o5)
    one = ta[:1, :1]
    o6, _ = k.gamma_rsample(one, rows, cols, seed, off)
    o7, _ = k.gamma_rsample(one.expand(rows, cols).contiguous(), rows, cols, seed, off)
    assert _bits_equal(o6, o7)


@pytest.mark.parametrize("a", gc.GAMMA_KS_A)
def test_gamma_draws_are_gamma_distributed(gpu, a):
    """Kolmogorov-Smirnov of 50 000 float64 draws against scipy.stats.gamma, either side of the boost at a = 1
    and from 0.05 to 1e5 (the oracle's draws at these seeds give p in [0.22, 0.80])."""
    from scipy import stats
    k = _k()
    ta = torch.full((1, 1), a, dtype=torch.float64, device=gpu)
    out, _ = k.gamma_rsample(ta, 1, gc.GAMMA_KS_N, gc.GAMMA_KS_SEED, gc.GAMMA_KS_OFFSET, want_grad=False)
    p = stats.kstest(out.cpu().numpy().reshape(-1), stats.gamma(a).cdf).pvalue
    print("\nKS a = %g: p = %.3f" % (a, p))
    assert p > gc.GAMMA_KS_P


# =======================================================================================================
# full-covariance guide
# =======================================================================================================

def _mvn_sample(inp, P, f32, gpu, given, seed=11, offset=5):
    """pa_mvn_tril_sample into carved buffers -> (z, logq, eps) tensors."""
    k = _k()
    from pyro_amd import _lib
    loc, rho, A, eps = (x.to(gpu, gc.dt(f32)).contiguous() for x in inp[:4])
    n = loc.numel()
    z, logq = Carved((P, n), f32, gpu), Carved((P,), f32, gpu)
    e = Carved((P, n), f32, gpu, eps if given else None)
    k.check(_lib.load().pa_mvn_tril_sample(k._dtype(loc), k._ptr(loc), k._ptr(rho), k._ptr(A), n, P, seed, offset,
                                           None, int(given), k._ptr(e.t), k._ptr(z.t), k._ptr(logq.t), k._stream()))
    torch.cuda.synchronize()
    assert z.intact() and logq.intact() and e.intact(), "a canary next to z, logq or eps was overwritten"
    return z.t, logq.t, e.t


def _mvn_bwd(inp, z, which, f32, gpu, accumulate):
    """pa_mvn_tril_sample_bwd into carved sinks (filled with 1.5 when accumulating) -> (d_loc, d_rho, d_A)."""
    k = _k()
    from pyro_amd import _lib
    loc, rho, A, eps, d_z, d_q = (x.to(gpu, gc.dt(f32)).contiguous() for x in inp)
    P, n = eps.shape
    init = 1.5 if accumulate else None
    fill = lambda shape: None if init is None else torch.full(shape, init)      # noqa: E731
    sinks = [Carved(s, f32, gpu, fill(s)) for s in ((n,), (n,), (n, n))]
    k.check(_lib.load().pa_mvn_tril_sample_bwd(k._dtype(loc), k._ptr(loc), k._ptr(rho), k._ptr(eps), k._ptr(z),
                                               k._ptr(d_z) if which[0] else None, k._ptr(d_q) if which[1] else None,
                                               n, P, *(k._ptr(s.t) for s in sinks), int(accumulate), k._stream()))
    torch.cuda.synchronize()
    assert all(s.intact() for s in sinks), "a canary next to a gradient of the guide was overwritten"
    return tuple(s.t for s in sinks)


def _mvn_path(n):
    return "row_per_thread" if n <= 128 else "wave_per_row"


def _mvn_one(n, P, f32, gpu, variant=None, backward=True, only=None):
    k = _k()
    label = "mvn/%s/%s" % (_mvn_path(n), gc.dname(f32))
    c = gc.mvn_case(n, P, f32, variant)
    inp = c["inp"]
    z, logq, eps = _mvn_sample(inp, P, f32, gpu, given=True)
    gc.mvn_check(label, (_np(z), _np(logq)), c, f32, only)
    # drawn instead of given: the stream's own normals, and then bit-equal z and logq; the wrapper agrees
    zd, qd, ed = _mvn_sample(inp, P, f32, gpu, given=False)
    assert _bits_equal(ed, k.philox_normal((P, n), gc.dt(f32), gpu, 11, 5))
    dev = [x.to(gpu, gc.dt(f32)).contiguous() for x in inp]
    zw, qw, ew = k.mvn_tril_sample(dev[0], dev[1], dev[2], P, seed=11, offset=5)
    assert _bits_equal(zw, zd) and _bits_equal(qw, qd) and _bits_equal(ew, ed)
    z2, q2, _ = k.mvn_tril_sample(dev[0], dev[1], dev[2], P, eps=ed.clone())
    assert _bits_equal(z2, zd) and _bits_equal(q2, qd)
    if not backward:
        return z, logq
    for which in ((True, True), (True, False), (False, True)):
        cw = gc.mvn_case(n, P, f32, variant, which)
        plain = _mvn_bwd(inp, z, which, f32, gpu, accumulate=False)
        gc.mvn_check(label, (None, None) + tuple(_np(x) for x in plain), cw, f32)
        upper = torch.ones(n, n, device=gpu).triu().bool()
        assert (plain[2][upper] == 0).all(), "d_A is not exactly 0 on and above the diagonal"
        acc = _mvn_bwd(inp, z, which, f32, gpu, accumulate=True)      # onto 1.5 everywhere, d_rho included
        c32 = cw["cpu32"] or (None,) * 5
        for what, a_, r, M, c in zip(gc.MVN_OUTPUTS[2:], acc, cw["ref"][2:], cw["M"][2:], c32[2:]):
            gc.check(label + "/sinks", what, _np(a_), r + 1.5, M + 1.5, f32, None if c is None else c + 1.5)
        assert (acc[2][upper] == 1.5).all(), "the accumulating form touched d_A on or above the diagonal"
    wd = k.mvn_tril_sample_bwd(dev[0], dev[1], dev[3], z, dev[4], dev[5])
    for a_, p_ in zip(wd, _mvn_bwd(inp, z, (True, True), f32, gpu, accumulate=False)):
        assert _bits_equal(a_, p_)
    return z, logq


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("n", gc.MVN_N)
def test_mvn_guide_grid(gpu, n, f32):
    """n either side of the 64-lane border and of the 128 / 129 switch between the two draw bodies, P on every
    remainder of the backward's unrolling by 8 particles; rho holds -30, 19.999, 20, 20.001 and 25; d_z alone,
    d_logq alone and both; plain and accumulating sinks (d_rho included) with canaries."""
    for P in gc.MVN_P:
        _mvn_one(n, P, f32, gpu)


def test_mvn_guide_underflowing_scale_f32(gpu):
    """rho = -200 in float32: softplus underflows to 0, z_i = loc_i and log q = +inf as the float32 CPU formula
    gives; every other z follows the rule."""
    n, P = 65, 5
    z, logq = _mvn_one(n, P, True, gpu, "underflow", backward=False, only=("z",))
    c = gc.mvn_case(n, P, True, "underflow")
    assert (gc.kind(_np(logq)) == gc.kind(c["cpu32"][1])).all() and bool(torch.isposinf(logq).all())
    assert np.array_equal(_np(z)[:, n // 2], np.broadcast_to(_np(c["inp"][0])[n // 2], (P,)))


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("n,P", [(65, 5), (129, 13)])
def test_mvn_guide_large_offset(gpu, n, P, f32):
    """loc = 1e4 with scales of 1e-3: scored per element, the offset does not swallow the draw."""
    z, _ = _mvn_one(n, P, f32, gpu, "offset")
    c = gc.mvn_case(n, P, f32, "offset")
    if not f32:
        spread = np.abs(c["ref"][0] - _np(c["inp"][0])).max()
        assert np.abs(_np(z) - c["ref"][0]).max() < 1e-6 * spread


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("n", [65, 128])
def test_mvn_draw_switches_bodies_above_128(gpu, n, f32):
    """Which body draws is visible only in the order of the additions.  Up to n = 128 a thread owns a row and keeps
    four partial sums (columns j mod 4): with A[i, 0] = B, A[i, 4] = -B (B = 2^30, in float64 2^60), A[i, 1] = 1
    and eps = 1 the first partial sum cancels exactly and the second holds the 1, so z_i = S (1 + 1) exactly.
    The wave-per-row body adds lane 1 to lane 0 first and loses the 1 beside B (z_i = S): either result is within
    the rule, so the grid above cannot tell where the switch sits -- this case pins it."""
    k = _k()
    d = gc.dt(f32)
    B = 2.0 ** 30 if f32 else 2.0 ** 60
    loc, rho = torch.zeros(n, dtype=d, device=gpu), torch.full((n,), 32.0, dtype=d, device=gpu)   # S = 32 exactly
    A = torch.zeros(n, n, dtype=d, device=gpu)
    A[n - 1, 0], A[n - 1, 4], A[n - 1, 1] = B, -B, 1.0
    z, _, _ = k.mvn_tril_sample(loc, rho, A, 1, eps=torch.ones(1, n, dtype=d, device=gpu))
    assert float(z[0, n - 1]) == 64.0 and float(z[0, 0]) == 32.0


# =======================================================================================================
# site kernels
# =======================================================================================================

def _site_one(rows, cols, lower, f32, gpu):
    k = _k()
    label = "site/%s/%s" % ("loop" if rows > 4 * 8 * _cus() else "rows", gc.dname(f32))
    c = gc.site_case(rows, cols, lower, f32)
    d = gc.dt(f32)
    u = c["u"].to(gpu, d)
    value, ld = k.exp_site_fwd(u, cols, lower)
    c32 = c["fwd32"] or (None, None)
    gc.check(label, "value", _np(value), c["fwd"][0], c["M_fwd"][0], f32, c32[0])
    gc.check(label, "ld", _np(ld), c["fwd"][1], c["M_fwd"][1], f32, c32[1])
    if f32:
        over = np.isinf(c32[0])
        assert (gc.kind(_np(value))[over] == gc.kind(c32[0])[over]).all()        # float32 exp overflows to +inf
    v2, none = k.exp_site_fwd(u, cols, lower, want_ld=False)
    assert none is None
    gc.check(label + "/value_only", "value", _np(v2), c["fwd"][0], c["M_fwd"][0], f32, c32[0])
    vin, gv, gl = c["value_in"].to(gpu, d), c["g_value"].to(gpu, d), c["g_ld"].to(gpu, d)
    for which in ((True, True), (True, False), (False, True)):
        ref, b32, M = gc.site_bwd_reference(c, which, f32)
        got = k.exp_site_bwd(vin, gv if which[0] else None, gl if which[1] else None, cols, lower)
        gc.check(label, "g_u", _np(got), ref, M, f32, b32)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("cols", gc.SITE_COLS)
def test_exp_site_kernels(gpu, cols, f32):
    """cols either side of the 64-lane wave, rows 1, 3, 5, lower 0, -2.5 and 1e6 (the cancellation of value -
    lower is scored by the rule), u in [-100, 80] with 3 % at 89 / 100 (float32 exp overflows), with and
    without the log-density, either gradient absent."""
    for rows in gc.SITE_ROWS:
        for lower in gc.SITE_LOWER:
            _site_one(rows, cols, lower, f32, gpu)


@pytest.mark.parametrize("f32", DTYPES)
def test_exp_site_rows_beyond_the_grid(gpu, f32):
    """More rows than 4 waves x 8 * CUs workgroups: the waves loop."""
    _site_one(gc.site_loop_rows(_cus()), 65, -2.5, f32, gpu)


@pytest.mark.parametrize("f32", DTYPES)
@pytest.mark.parametrize("P,n", gc.SCORE_SHAPES + (gc.SCORE_CAP_SHAPE,))
def test_meanfield_score(gpu, P, n, f32):
    """pa_meanfield_score: n below, at and above the 256 threads of the modular column walk, and P * n just
    above the cap of 1024 blocks; the total and -coef P / scale per element; repeated calls bit-equal."""
    from pyro_amd import _lib
    k = _k()
    c = gc.score_case(P, n, f32)
    d = gc.dt(f32)
    z, loc, scale = (c[w].to(gpu, d).contiguous() for w in ("z", "loc", "scale"))
    partial, gscale = k.meanfield_score(z, loc, scale, P, gc.SCORE_COEF)
    nb = int(_lib.load().pa_meanfield_score_blocks(P, n))
    assert partial.shape == (nb,) and nb == min(1024, max(1, (P * n + 4095) // 4096))
    label = "score/%s/%s" % ("capped" if P * n > 1024 * 4096 else "blocks", gc.dname(f32))
    gc.score_check(label, _np(partial).sum(), _np(gscale), c, f32)
    again, g2 = k.meanfield_score(z, loc, scale, P, gc.SCORE_COEF)
    assert _bits_equal(partial, again) and _bits_equal(gscale, g2)
