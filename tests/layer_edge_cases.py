"""Grids, input builders, the float64 reference and the ONE tolerance rule of the matrix-core layer
kernels (csrc/tall.hip, csrc/bow.hip): shared by test_layer_edges_gpu.py, test_layer_edges_host.py and
the pinned-wave-count worker tests/layer_worker.py.

Reference: the operation in float64 from the f32 inputs (torch float64; on the CPU for small cases, on
the device -- rocBLAS, independent of the code under test -- for large ones).  Fused forms: float64 of
the same formula, sigmoid(G Wm + b), and g * (1 - y) * y from the f32 y the kernel is given.

Tolerance, per element, no max-norm term (u = 2^-24):

    |got_ij - ref_ij| <= c u (|A| |B|)_ij + |bias_j| u

    c = 1 + 4 T(inner) [* max(1, sqrt(inner) / 30) when inner > 128]

  1      the three dropped piece products (x2 w3, x3 w2, x3 w3): at most 1 u per term (0.77 u seen over
         2e5 normal pairs; test_layer_edges_host.py holds it under 1);
  T      the largest ratio err / (u |A||B|) of TORCH'S OWN f32 product (tx @ tW.t(), tg.t() @ tx) on the
         same grid against the same float64 reference, per inner-dimension class; the kernels get four
         times that (six additions per term where an f32 GEMM makes one: sqrt(6) in a random-walk model,
         rounded up);
  growth the batch-long sums (wgrad, tsgemm, bow backward; inner = B > 128) keep the sqrt(B) / 30 growth of
         test_tall_skinny_weight_gradient_product;
  y_mul  the operand A = g * (1 - y) * y is formed in f32 by three rounded operations where the reference forms it
         in float64; that is inside the same c (no extra term);
  bias   one more f32 addition.
A fused sigmoid output is held to c u (|A||B|) / 4 + |bias| u / 4 + 3e-6 (sigmoid' <= 1/4; 3e-6 is the
tolerance the existing tests give the hardware exp2 / rcp).

c must stay below 32 for inner <= 128: a lost third piece is 2^-16 relative in one operand, up to 256 u,
and a looser rule could not see one on mixed-sign data.

Measured on the MI355X (256 CUs), largest err / (u |A||B|) over the grids below:

    class                                torch f32 (T)   kernels   c of the rule
    inner <= 128                         7.66            6.91      31.64
    inner > 128, / max(1, sqrt / 30)     7.20            4.91      29.8 x max(1, sqrt(inner) / 30)

(test_zz_measured_constants prints both columns.)  Results below the f32 normal range are not part of any grid:
the hardware flushes f32 denormals, and an operand g * (1 - y) * y that underflows is a limit of f32, not of
the kernels.

Integer cases need no tolerance: integer-valued operands of magnitude <= 8 (one bf16 piece each) with
sums under 2^24 make every piece product and every partial sum exact in f32, so the result must
torch.equal the int64 product.  That is the indexing test.

Every input sits as a contiguous view inside a larger NaN-filled buffer (16-byte aligned offset unless
the case is about alignment), every output of a direct C-ABI call inside a sentinel-filled one whose
sentinels are checked afterwards.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
T_SHORT = 7.66       # torch's own f32 product, inner <= 128   (see the table above)
T_LONG = 7.20        # torch's own f32 product, inner > 128, after the sqrt(inner) / 30 growth
SIGMOID_ATOL = 3e-6
SENTINEL = -1.2345e30
PAD = 64             # floats of NaN / sentinel on either side of a tensor
BOW_MAX_COUNT = 256


def c_rule(inner):
    """The accumulation constant c of the rule (below 32 for inner <= 128)."""
    return 1.0 + 4.0 * (T_SHORT if inner <= 128 else T_LONG * max(1.0, math.sqrt(inner) / 30.0))


# ---- builders ------------------------------------------------------------------------------------
def embed(t, offset=4, fill=float("nan")):
    """A contiguous copy of ``t`` inside a larger buffer filled with ``fill``, ``offset`` floats from its
    start (4 = 16-byte aligned, 5 = odd: 4-byte aligned only)."""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=t.device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(shape, g, dev):
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def randint8(shape, g, dev):
    return torch.randint(-8, 9, shape, generator=g, device=dev).float()


def pow2_scales(n, g, dev, lo=-20, hi=20):
    return torch.exp2(torch.rand((n,), generator=g, device=dev) * (hi - lo) + lo).float()


def ref_matmul(a, b):
    """a @ b in float64 (CPU for small products, the device otherwise); returns (product, |a| @ |b|) on a's device."""
    dev = a.device
    small = a.shape[0] * a.shape[1] * b.shape[1] <= (1 << 22)
    a64, b64 = a.double(), b.double()
    if small:
        a64, b64 = a64.cpu(), b64.cpu()
    return (a64 @ b64).to(dev), (a64.abs() @ b64.abs()).to(dev)


def dsig64(g, y):
    g, y = g.double(), y.double()
    return g * (1.0 - y) * y


def verdict(got, ref, absprod, c, bias=None, sigmoid=False, what=""):
    """The rule.  Returns dict(ok, ratio, what, msg): ratio = the largest (err - |bias| u) / (u |A||B|) (for a sigmoid
    output: of what exceeds the 3e-6 as well), the quantity of which c is the limit."""
    got = got.double()
    unit = U * absprod
    free = torch.zeros_like(unit)
    if bias is not None:
        free = free + bias.double().abs() * U
    if sigmoid:
        unit, free = unit / 4, free / 4 + SIGMOID_ATOL
    lim = c * unit + free
    err = (got - ref).abs()
    finite = torch.isfinite(got).all().item() and torch.isfinite(ref).all().item()
    excess = (err - free).clamp_min(0.0)
    ratio = torch.where(unit > 0, excess / unit.clamp_min(1e-300), torch.where(excess > 0, math.inf, 0.0))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    ok = bool(finite and bool((err <= lim).all()))
    msg = ""
    if not ok:
        i = int(ratio.argmax())
        msg = "%s: worst element %s: got %r ref %r, err = %.3g units (limit c = %.3g); %d of %d outside" % (
            what, tuple(int(x) for x in np.unravel_index(i, tuple(got.shape))), float(got.reshape(-1)[i]),
            float(ref.reshape(-1)[i]), worst, c, int((~(err <= lim)).sum()), got.numel())
    return {"ok": ok, "ratio": worst, "what": what, "msg": msg}


RATIOS = {}          # class -> [torch's largest ratio, the kernels' largest ratio]  (filled as cases run)


def note(cls, torch_ratio, kernel_ratio):
    r = RATIOS.setdefault(cls, [0.0, 0.0])
    r[0], r[1] = max(r[0], torch_ratio), max(r[1], kernel_ratio)


def torch_ratio(a32, b32, ref, absprod):
    """err / (u |A||B|) of torch's own f32 product of the same operands."""
    err = ((a32 @ b32).double() - ref).abs()
    return float((err / (U * absprod).clamp_min(1e-300)).max())


def inner_class(inner):
    return "inner <= 128" if inner <= 128 else "inner = B > 128 (after growth)"


def growth(inner):
    return 1.0 if inner <= 128 else max(1.0, math.sqrt(inner) / 30.0)


# ---- direct C-ABI calls with sentinel-guarded outputs ---------------------------------------------------
def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def _guards_intact(buf, n):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


def tall_linear_raw(g, w_view, w_rs, w_cs, C, bias=None, y_mul=None, sigmoid=False):
    """pa_tall_linear_act on raw pointers (any weight strides / alignment); checks the output's guards."""
    from pyro_amd import _lib, kernels as k
    B, R = g.shape
    assert g.is_contiguous() and (y_mul is None or y_mul.is_contiguous())
    buf, out = _guarded((B, C), g.device)
    k.check(_lib.load().pa_tall_linear_act(k._ptr(g), B, R, w_view.data_ptr(), int(w_rs), int(w_cs), int(C),
                                           k._ptr(bias), k._ptr(y_mul), int(bool(sigmoid)), out.data_ptr(),
                                           k._stream()))
    torch.cuda.synchronize()
    assert _guards_intact(buf, B * C), "tall_linear wrote outside its output"
    return out


def tall_wgrad_raw(g, x, y_mul=None, want_bias=True):
    from pyro_amd import _lib, kernels as k
    B, R = g.shape
    K = x.shape[1]
    lib = _lib.load()
    nbytes = lib.pa_tall_wgrad_workspace(B, R, K)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=g.device)
    bw, dW = _guarded((R, K), g.device)
    bb, db = _guarded((R,), g.device)
    k.check(lib.pa_tall_wgrad_act(k._ptr(g), k._ptr(x), k._ptr(y_mul), B, R, K, dW.data_ptr(),
                                  db.data_ptr() if want_bias else None, k._ptr(ws), nbytes, k._stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bw, R * K) and _guards_intact(bb, R), "tall_wgrad wrote outside its outputs"
    if not want_bias:
        assert bool((db == SENTINEL).all()), "tall_wgrad wrote a bias gradient nobody asked for"
    return dW, (db if want_bias else None)


# ---- paths ------------------------------------------------------------------------------------
def linear_case_path(case, operands):
    from pyro_amd import kernels as k
    g, w_view, w_rs, w_cs, _wm, _bias, y = operands
    return k.tall_linear_path(case["B"], case["R"], case["C"], w_rs, w_cs, g, y, w_view)


def b16(cus):
    """The first B that takes the sixteen-wave form of tall_linear: ceil(B / 32) = 4 CUs."""
    return 32 * (4 * cus - 1) + 1


def bw8(cus, nrt):
    """The first B that takes the eight-wave form of tall_wgrad: ceil(B / 16) nrt >= 24 CUs."""
    return 16 * (-(-24 * cus // nrt) - 1) + 1


# pairs (R, C) on both sides of every (NKS, NCT) boundary: nks = ceil(R / 16), nct = ceil(C / 32);
# (1, 4): R <= 16; (8, 1): R > 16, C <= 32; (7, 4): 16 < R <= 112, C > 32; (8, 4): R > 112, C > 32
LINEAR_RC = [(1, 1), (3, 127), (4, 31), (15, 33), (16, 128), (17, 32), (17, 33), (31, 17), (32, 32), (33, 15),
             (100, 100), (100, 8), (112, 33), (112, 128), (113, 32), (113, 33), (127, 3), (128, 32), (128, 100),
             (128, 128), (16, 4), (100, 32), (128, 1)]
LINEAR_B_SMALL = [1, 31, 32, 33, 127, 129, 4100]
# the shapes that reach every (NKS, NCT) in the sixteen-wave form (R % 4 == 0), staged (a contiguous weight that
# fits) and not
LINEAR_RC_16 = [(4, 31), (16, 128), (32, 32), (100, 8), (100, 100), (112, 128), (128, 100), (128, 128), (128, 32)]


def linear_cases(cus):
    """dicts(B, R, C, orient, bias, sigmoid, ymul, wkind, gkind, scale): the grid of pa_tall_linear_act."""
    cases = []

    def add(B, R, C, orient="fwd", bias=True, sigmoid=False, ymul=False, wkind="contig", gkind="aligned",
            scale="none"):
        cases.append(dict(B=B, R=R, C=C, orient=orient, bias=bias, sigmoid=sigmoid, ymul=ymul, wkind=wkind,
                          gkind=gkind, scale=scale))

    # every (R, C) pair at a few small B, both orientations; the fused forms ride along in rotation
    for i, (R, C) in enumerate(LINEAR_RC):
        for j, B in enumerate(LINEAR_B_SMALL):
            if (i + j) % 3 == 0 or B in (33, 4100):
                add(B, R, C, orient=("fwd", "dx")[(i + j) % 2], bias=(i + j) % 2 == 0, sigmoid=(i + j) % 4 == 0,
                    ymul=(i + j) % 5 == 0)
    # the sixteen-wave threshold from both sides, 1e5; staged / unstaged by shape; slices and odd offsets
    first = b16(cus)
    for i, (R, C) in enumerate(LINEAR_RC_16):
        for B in (first - 1, first, 100_000):
            add(B, R, C, orient="fwd", bias=i % 2 == 0, sigmoid=i % 3 == 0)
            add(B, R, C, orient="dx", bias=False, ymul=i % 2 == 1)
        add(first, R, C, orient="fwd", wkind="slice")             # not contiguous: never staged; vector reads
        add(first, R, C, orient="dx", wkind="slice", ymul=True)   # not contiguous, w_rs != 1: gathers
        add(first, R, C, orient="fwd", wkind="odd")               # unaligned weight: no stage, no vector reads
        add(first, R, C, orient="fwd", gkind="odd")               # unaligned G: four waves, float4 row loads
        add(first, R, C, orient="dx", gkind="oddy", ymul=True)    # unaligned y_mul alone
    for R, C in ((100, 100), (128, 128), (17, 33), (16, 128), (3, 127)):
        for B in (129, 4100):
            add(B, R, C, orient="fwd", wkind="slice")
            add(B, R, C, orient="dx", wkind="odd", gkind="odd", ymul=True)
            add(B, R, C, orient="fwd", scale="pow2")
            add(B, R, C, orient="dx", scale="pow2", bias=False)
            add(B, R, C, orient="fwd", scale="cancel", bias=False)
    # the benchmark's own layers on the staged path, plain and fused, scaled and cancelling
    for R, C in ((100, 100), (100, 8)):
        add(100_000, R, C, orient="fwd", sigmoid=True)
        add(100_000, C, R, orient="dx", bias=False, ymul=True)
        add(100_000, R, C, orient="fwd", scale="pow2")
        add(100_000, R, C, orient="fwd", scale="cancel", bias=False)
    return cases


def linear_operands(case, dev, ints=False, seed=0):
    """(G, w_view, w_rs, w_cs, Wm [R, C] dense f32, bias, y_mul) of a case; Wm[r][c] = w_view.flat[r w_rs + c w_cs]."""
    B, R, C = case["B"], case["R"], case["C"]
    g = gen(1000 * seed + B + 131 * R + 17 * C, dev)
    draw = randint8 if ints else randn
    G = draw((B, R), g, dev)
    rows, cols = (C, R) if case["orient"] == "fwd" else (R, C)      # the nn.Linear weight [rows, cols]
    W = draw((rows, cols), g, dev)
    if not ints:
        W = W / math.sqrt(R)
    if case["scale"] == "pow2" and not ints:
        G = G * pow2_scales(B, g, dev)[:, None]
        cs = pow2_scales(C, g, dev)
        W = W * (cs[:, None] if case["orient"] == "fwd" else cs[None, :])
    if case["scale"] == "cancel" and not ints and R >= 3:
        # rows [t, -t, small, ...]: the two leading terms cancel in every output
        G[:, 1] = -G[:, 0]
        if case["orient"] == "fwd":
            W[:, 1] = W[:, 0]
            W[:, 2:] *= 2.0 ** -12
        else:
            W[1, :] = W[0, :]
            W[2:, :] *= 2.0 ** -12
    Wm = (W.t() if case["orient"] == "fwd" else W).contiguous()
    if case["wkind"] == "slice":
        wide = torch.full((rows, cols + 8), float("nan"), device=dev)
        w_view = wide[:, 4:4 + cols]
        w_view.copy_(W)
        ld = cols + 8
    else:
        w_view = embed(W, offset=5 if case["wkind"] == "odd" else 4)
        ld = cols
    w_rs, w_cs = (1, ld) if case["orient"] == "fwd" else (ld, 1)
    bias = embed(draw((C,), g, dev)) if case["bias"] else None
    y = None
    if case["ymul"]:
        y = torch.rand((B, R), generator=g, device=dev)
        if ints:
            y = torch.full_like(y, 0.5)              # g (1 - 1/2) 1/2 = g / 4: exact
        y = embed(y, offset=5 if case["gkind"] in ("odd", "oddy") else 4)
    G = embed(G, offset=5 if case["gkind"] == "odd" else 4)
    return G, w_view, w_rs, w_cs, Wm, bias, y


def run_linear_case(case, dev, ints=False):
    """Launch the case and score it: the rule for real data, torch.equal of the int64 product for integers."""
    ops = linear_operands(case, dev, ints)
    v = _score_linear_case(case, ops, ints)
    v["path"] = linear_case_path(case, ops)          # from the pointers the launcher was handed
    return v


def _score_linear_case(case, ops, ints):
    G, w_view, w_rs, w_cs, Wm, bias, y = ops
    sig = case["sigmoid"] and not ints
    out = tall_linear_raw(G, w_view, w_rs, w_cs, case["C"], bias, y, sig)
    what = "tall_linear %r%s" % (case, " ints" if ints else "")
    if ints:
        ref = (G.double() @ Wm.double()).float() / (4.0 if y is not None else 1.0)   # (y = 1/2: the operand is g / 4)
        if bias is not None:
            ref = ref + bias
        ok = torch.equal(out, ref)
        return {"ok": ok, "ratio": 0.0, "what": what,
                "msg": "" if ok else "%s: %d elements differ from the integer product" % (what, int((out != ref).sum()))}
    A = G.double() if y is None else dsig64(G, y)
    ref, absprod = ref_matmul(A, Wm)
    tr = torch_ratio(A.float(), Wm, ref, absprod)
    if bias is not None:
        ref = ref + bias.double()
    if sig:
        ref = torch.sigmoid(ref)
    v = verdict(out, ref, absprod, c_rule(case["R"]), bias, sig, what)
    if not sig:
        note(inner_class(case["R"]), tr, v["ratio"])
    return v


# ---- wgrad ------------------------------------------------------------------------------------
WGRAD_RK = [(1, 1), (31, 128), (32, 32), (33, 33), (64, 64), (65, 65), (96, 96), (97, 97), (128, 128), (128, 1),
            (1, 128), (64, 97), (96, 32), (31, 33), (100, 100), (8, 100), (100, 8), (65, 1)]


def wgrad_cases(cus):
    cases = []

    def add(B, R, K, ymul=False, want_bias=True, scale="none"):
        cases.append(dict(B=B, R=R, K=K, ymul=ymul, want_bias=want_bias, scale=scale))

    for i, (R, K) in enumerate(WGRAD_RK):
        nrt = -(-R // 32)
        nrt = 4 if nrt == 3 else nrt
        t8 = bw8(cus, nrt)
        for j, B in enumerate((1, 15, 16, 17, 4097, t8 - 1, t8, 100_000)):
            if (i + j) % 3 == 0 or B in (17, t8):
                add(B, R, K, ymul=(i + j) % 2 == 0, want_bias=(i + j) % 4 != 3,
                    scale="pow2" if (i + j) % 5 == 0 else "none")
    for R, K in ((100, 100), (8, 100)):                 # the benchmark's layers
        add(100_000, R, K, ymul=True)
        add(100_000, R, K, scale="pow2")
    return cases


def wgrad_operands(case, dev, ints=False):
    B, R, K = case["B"], case["R"], case["K"]
    g = gen(7 + B + 131 * R + 17 * K, dev)
    draw = randint8 if ints else randn
    G, X = draw((B, R), g, dev), draw((B, K), g, dev)
    if case["scale"] == "pow2" and not ints:
        G = G * pow2_scales(R, g, dev)[None, :]
        X = X * pow2_scales(K, g, dev)[None, :]
    y = None
    if case["ymul"]:
        y = torch.rand((B, R), generator=g, device=dev)
        if ints:
            y = torch.full_like(y, 0.5)
        y = embed(y)
    return embed(G), embed(X), y


def run_wgrad_case(case, dev, ints=False):
    G, X, y = wgrad_operands(case, dev, ints)
    dW, db = tall_wgrad_raw(G, X, y, case["want_bias"])
    dW2, db2 = tall_wgrad_raw(G, X, y, case["want_bias"])
    what = "tall_wgrad %r%s" % (case, " ints" if ints else "")
    if not torch.equal(dW, dW2) or (db is not None and not torch.equal(db, db2)):
        return {"ok": False, "ratio": math.inf, "what": what, "msg": what + ": two runs differ bitwise"}
    B = case["B"]
    if ints:
        div = 4.0 if y is not None else 1.0
        ok = torch.equal(dW, (G.double().t() @ X.double()).float() / div)
        if db is not None:
            ok = ok and torch.equal(db, G.double().sum(0).float() / div)
        return {"ok": ok, "ratio": 0.0, "what": what, "msg": "" if ok else what + ": differs from the integer product"}
    A = G.double() if y is None else dsig64(G, y)
    ref, absprod = ref_matmul(A.t(), X)
    v = verdict(dW, ref, absprod, c_rule(B), what=what + " dW")
    note(inner_class(B), torch_ratio(A.float().t(), X, ref, absprod) / growth(B), v["ratio"] / growth(B))
    if db is not None and v["ok"]:
        v2 = verdict(db, A.sum(0), A.abs().sum(0), c_rule(B), what=what + " db")
        v2["ratio"] = max(v["ratio"], v2["ratio"])
        return v2
    return v


# ---- bag of words ----------------------------------------------------------------------------------
def bow_ksplit_edge(cus, V):
    """The largest B at which every k-step of 16 documents still has a workgroup of its own in the backward
    (bow_ksplit = the k-step count); from B + 1 on a workgroup sums two.  This restates bow_ksplit() of
    csrc/bow.hip; test_bag_of_words_edge_straddles_a_change_of_ksplit holds it against the launcher's own
    pa_bow_workspace, which is sized by the real bow_ksplit."""
    return 16 * (cus * 3 // (V // 128))


def bow_ksplit_of(B, V, H=100):
    """bow_ksplit as the launcher computes it, read back from pa_bow_workspace = d planes + ksplit partial tiles."""
    from pyro_amd import _lib
    Bp = (B + 31) // 32 * 32
    dplanes = 3 * 4 * (Bp // 16) * 64 * 16
    part = int(_lib.load().pa_bow_workspace(B, V, H)) - dplanes
    assert part > 0 and part % (128 * V * 4) == 0, (B, V, part)
    return part // (128 * V * 4)


def bow_cases(cus):
    cases = []
    HV = [(1, 128), (31, 384), (32, 1024), (33, 128), (100, 1024), (128, 384), (100, 128), (128, 1024)]
    Bs = [1, 31, 33, 255, 256, 257, 3000]
    for i, (H, V) in enumerate(HV):
        for j, B in enumerate(Bs):
            if (i + j) % 3 == 0 or B in (33, 257):
                cases.append(dict(B=B, H=H, V=V, Wd=(7, 64, 30)[(i + j) % 3], corpus="random"))
    for V in (1024, 384):
        e = bow_ksplit_edge(cus, V)
        cases.append(dict(B=e, H=100, V=V, Wd=16, corpus="random"))
        cases.append(dict(B=e + 1, H=100, V=V, Wd=16, corpus="random"))
    cases.append(dict(B=257, H=100, V=384, Wd=BOW_MAX_COUNT, corpus="one-word"))    # a document of one word 256 times
    cases.append(dict(B=300, H=33, V=128, Wd=1, corpus="random"))
    return cases


def bow_operands(case, dev, ints=False):
    B, H, V, Wd = case["B"], case["H"], case["V"], case["Wd"]
    g = gen(3 + B + 131 * H + V + Wd, dev)
    words = torch.randint(0, V, (Wd, B), generator=g, device=dev)
    if case["corpus"] == "one-word":
        words[:, 0] = 5
        words[:, B - 1] = V - 1
    if ints:
        W = torch.randint(-8, 9, (H, V), generator=g, device=dev).float()
        d = torch.randint(-8, 9, (B, H), generator=g, device=dev).float()
        bias = torch.randint(-8, 9, (H,), generator=g, device=dev).float()
    else:
        W = randn((H, V), g, dev) * 0.05 * pow2_scales(H, g, dev, -10, 10)[:, None]
        d = randn((B, H), g, dev) * pow2_scales(H, g, dev, -10, 10)[None, :]
        bias = randn((H,), g, dev)
    counts = torch.zeros((V, B), device=dev).scatter_add_(0, words, torch.ones(words.shape, device=dev))
    # (the sigmoid output that the backward reads comes from a weight of ordinary size: behind the scaled one y
    #  saturates and d (1 - y) y underflows f32 -- a limit of the format, not of the kernels)
    Wy = embed(W) if ints else embed(randn((H, V), g, dev) * 0.05)
    return words, counts, embed(W), embed(bias), embed(d), Wy


# ---- tsgemm ------------------------------------------------------------------------------------
def tsgemm_cases():
    MN = [(1, 1), (31, 128), (32, 32), (33, 31), (128, 128), (128, 1), (1, 33)]
    Bs = [1, 31, 33, 4097, 100_000]
    return [dict(B=B, M=M, N=N) for i, (M, N) in enumerate(MN) for j, B in enumerate(Bs)
            if (i + j) % 2 == 0 or B == 33]


# ---- the split, as torch does it on the CPU ---------------------------------------------------------
def split3(x):
    """x = p1 + p2 + p3 with three round-to-nearest bf16 pieces, residuals in f32: glm_bf16.h's split_pair."""
    p1 = x.to(torch.bfloat16).float()
    r = x - p1
    p2 = r.to(torch.bfloat16).float()
    q = r - p2
    p3 = q.to(torch.bfloat16).float()
    return p1, p2, p3


SPLIT_EXPONENTS = (-126, -118, -110, -102, -90, 0, 100, 120, 126)
SPLIT_MUST_HOLD = (-100, 120)        # inside: the rule holds; outside: measured and pinned


def mantissas(shape, g, dev):
    """Random signs times random f32 values in [1, 2) with all 24 bits in play."""
    m = 1.0 + torch.rand(shape, generator=g, device=dev, dtype=torch.float64)
    s = torch.randint(0, 2, shape, generator=g, device=dev).double() * 2 - 1
    return (m * s).float()
