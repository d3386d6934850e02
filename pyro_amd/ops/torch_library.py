"""The kernels as torch dispatcher ops (``torch.ops.pyro_amd.*``).

SURVEY 8(b) asks that the backend's numerics appear to torch as custom ops so that they survive
``torch.jit.trace`` (what the reference's ``JitTrace_ELBO`` is built on, pyro/ops/jit.py:104-109,
pyro/infer/trace_elbo.py:162-257) and ``torch.compile``: a ctypes launch is invisible to a tracer, the
tensors it fills would be frozen into the graph as constants.  Two layers:

* ``csrc/torch_ops.cpp`` (``TORCH_LIBRARY``, C++ over the extern-"C" launchers): the observed GLM site
  ``glm_bernoulli[_planes]`` + its backward ``glm_chain``, ``glm_pack_planes``, and the flat optimizer
  update ``adam_step``.  This module adds their shape functions (``register_fake``) and autograd
  formulas (``register_autograd``).

* every other kernel-backed operation of a step is a ``torch.autograd.Function`` of this package
  (``distributions/fused.py``, ``ops/contract.py``, ``ops/lazy.py``: the mean-field guide draw, the
  multi-site ELBO assembly, the single-site sums, the Dirichlet / Gamma / Normal draws, the
  AutoMultivariateNormal draw, the LDA factor, the log-sum-exp elimination step, the chain kernel,
  the bag-of-words and tall-batch layers).  ``dispatcher_op(name)`` registers each of them as a pair of
  NAMED dispatcher ops, ``pyro_amd::<name>`` and ``pyro_amd::<name>_bwd``, with the schema
  ``(Tensor[] tensors, int spec) -> Tensor[]``, a shape function and an autograd formula that
  connects the two.  ``tensors`` are ALL tensor arguments of the call (whatever their nesting);
  ``spec`` names the call's non-tensor arguments -- distribution ids, broadcast frames, Philox offsets,
  scales -- in a table of this process (the reference's traced functions are not serialisable either:
  they close over the model).  The op bodies run the Function's own ``forward`` / ``backward``, i.e.
  the very launches the eager path makes, so a traced graph and the eager step cannot drift apart.

Routing: ``Function.apply`` goes through the dispatcher op while a tracer is recording (or inside
``routing()``); the un-traced hot path keeps calling the launchers directly (its chained tail and
gradient sinks are wired to them).
"""
import os

import torch

from .. import _lib, kernels

_LIB = os.path.join(os.path.dirname(_lib.__file__), "lib", "libpyro_amd_torch.so")
_state = {"loaded": None}


def available():
    """True once libpyro_amd_torch.so is loaded (built by csrc/build.py next to libpyro_amd.so)."""
    if _state["loaded"] is None:
        _state["loaded"] = False
        if os.path.exists(_LIB) and os.environ.get("PYRO_AMD_TORCH_OPS", "1") != "0":
            _lib.load()                      # libpyro_amd.so first: the shim links against it
            torch.ops.load_library(_LIB)
            _register()
            _state["loaded"] = True
    return _state["loaded"]


def _register():
    lib = torch.library

    @lib.register_fake("pyro_amd::glm_pack_planes")
    def _(X, format):
        n = _lib.load().pa_glm_planes_bytes(int(format), X.shape[0], X.shape[1])
        return X.new_empty((max(n, 16),), dtype=torch.uint8)

    def _four(w, nbytes):
        P = w.shape[0]
        return (w.new_empty((P,)), w.new_empty(tuple(w.shape)), w.new_empty((P,)),
                w.new_empty((max(int(nbytes), 1),), dtype=torch.uint8))

    @lib.register_fake("pyro_amd::glm_bernoulli_planes")
    def _(planes, y, w, b, scale, N, D, format, moments=None):
        return _four(w, _lib.load().pa_glm_bernoulli_planes_workspace(int(N), int(D), w.shape[0]))

    @lib.register_fake("pyro_amd::glm_bernoulli")
    def _(X, y, w, b, mask, scale):
        return _four(w, _lib.load().pa_glm_bernoulli_workspace(X.shape[0], X.shape[1], w.shape[0]))

    @lib.register_fake("pyro_amd::glm_chain")
    def _(g, gw, gb):
        return torch.empty_like(gw), torch.empty_like(gb)

    @lib.register_fake("pyro_amd::adam_step")
    def _(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, clip_norm, lrd,
          clipped, zero_grad):
        return None

    # ---- shape functions of the typed ops (csrc/torch_ops.cpp, round 6) --------------------------------------
    def _frame(value):
        cols = value.shape[-1] if value.dim() else 1
        return (value.numel() // cols if cols else 0), cols

    @lib.register_fake("pyro_amd::dist_log_prob_sum")
    def _(dist, value, p0, p1, mask, scale):
        return value.new_empty((_frame(value)[0],)), value.new_empty(())

    @lib.register_fake("pyro_amd::multi_log_prob_sum")
    def _(dist, value, p0, p1, coef, coef_all):
        return value[0].new_empty(())

    @lib.register_fake("pyro_amd::meanfield_normal_sample")
    def _(loc, rho, P, seed, offsets, offset_dev):
        z = [t.new_empty((P, t.numel())) for t in loc]
        return z, [t.new_empty((t.numel(),)) for t in loc], [t.new_empty((P, t.numel())) for t in loc]

    @lib.register_fake("pyro_amd::exp_site")
    def _(u, lower):
        return torch.empty_like(u), u.new_empty((_frame(u)[0],))

    @lib.register_fake("pyro_amd::exp_site_bwd")
    def _(value, g_value, g_log_density, lower):
        return torch.empty_like(value)

    @lib.register_fake("pyro_amd::mvn_tril_sample")
    def _(loc, rho, A, P, seed, offset, offset_dev):
        n = loc.numel()
        return loc.new_empty((P, n)), loc.new_empty((P, n)), loc.new_empty((P,))

    @lib.register_fake("pyro_amd::logsumexp_terms")
    def _(terms, sizes, rdim):
        return terms[0].new_empty([n for d, n in enumerate(sizes) if d != rdim])

    @lib.register_fake("pyro_amd::logchain")
    def _(unary, pairwise):
        B, T, K = unary.shape
        return unary.new_empty((B,)), torch.empty_like(unary), unary.new_empty((B, max(T - 1, 0), K, K))

    @lib.register_fake("pyro_amd::logchain_decode")
    def _(unary, pairwise, mode, seed, offset, offset_dev, step_blocks):
        B, T, _K = unary.shape
        return unary.new_empty((B, T), dtype=torch.int64), unary.new_empty((B,))

    @lib.register_fake("pyro_amd::gaussian_hmm")
    def _(m0, P0, trans, trans_loc, trans_cov, obs, obs_loc, obs_cov, x, need_grads):
        B, T, o = x.shape
        h = m0.shape[-1]
        grads = []
        if need_grads:
            steps = [t.shape[1] for t in (trans, trans_loc, trans_cov, obs, obs_loc, obs_cov)]
            grads = [x.new_empty((B, h)), x.new_empty((B, h, h)), x.new_empty((B, steps[0], h, h)),
                     x.new_empty((B, steps[1], h)), x.new_empty((B, steps[2], h, h)), x.new_empty((B, steps[3], h, o)),
                     x.new_empty((B, steps[4], o)), x.new_empty((B, steps[5], o, o)), x.new_empty((B, T, o))]
        return x.new_empty((B,)), x.new_empty((B, h)), x.new_empty((B, h, h)), grads

    @lib.register_fake("pyro_amd::gamma_gaussian_hmm")
    def _(concentration, rate, m0, P0, trans, trans_loc, trans_cov, obs, obs_loc, obs_cov, x, need_grads):
        B, T, o = x.shape
        h = m0.shape[-1]
        grads = []
        if need_grads:
            steps = [t.shape[1] for t in (trans, trans_loc, trans_cov, obs, obs_loc, obs_cov)]
            grads = [x.new_empty((B, h)), x.new_empty((B, h, h)), x.new_empty((B, steps[0], h, h)),
                     x.new_empty((B, steps[1], h)), x.new_empty((B, steps[2], h, h)), x.new_empty((B, steps[3], h, o)),
                     x.new_empty((B, steps[4], o)), x.new_empty((B, steps[5], o, o)), x.new_empty((B, T, o))]
        return x.new_empty((B,)), x.new_empty((B,)), x.new_empty((B, h)), x.new_empty((B, h, h)), grads

    @lib.register_fake("pyro_amd::gaussian_hmm_sample")
    def _(m0, P0, trans, trans_loc, trans_cov, obs, obs_loc, obs_cov, x, eps, need_maps):
        B, T, _o = x.shape
        h = m0.shape[-1]
        maps = [x.new_empty((B, T, h)), x.new_empty((B, T, h, h)), x.new_empty((B, T, h, h))] if need_maps else []
        return x.new_empty((eps.shape[0], B, T, h)), maps

    @lib.register_fake("pyro_amd::gaussian_hmm_smooth")
    def _(m0, P0, trans, trans_loc, trans_cov, obs, obs_loc, obs_cov, x, need_cross):
        B, T, _o = x.shape
        h = m0.shape[-1]
        cross = [x.new_empty((B, T - 1, h, h))] if need_cross else []
        return x.new_empty((B, T, h)), x.new_empty((B, T, h, h)), cross

    @lib.register_fake("pyro_amd::gaussian_hmm_draw")
    def _(m0, P0, trans, trans_loc, trans_cov, obs, obs_loc, obs_cov, T, eps0, eps_z, eps_x, need_states):
        S, B, h = eps0.shape
        states = [eps0.new_empty((S, B, T, h))] if need_states else []
        return eps0.new_empty((S, B, T, obs.shape[-1])), states

    @lib.register_fake("pyro_amd::linear_hmm_draw")
    def _(trans, obs, T, init, e, n, need_states):
        S, B, h = init.shape
        states = [init.new_empty((S, B, T, h))] if need_states else []
        return init.new_empty((S, B, T, obs.shape[-1])), states

    @lib.register_fake("pyro_amd::forecast_scores")
    def _(pred, truth):
        return torch.empty_like(truth), torch.empty_like(truth), torch.empty_like(truth)

    @lib.register_fake("pyro_amd::time_transform")
    def _(x, op, dim):
        return torch.empty_like(x)

    @lib.register_fake("pyro_amd::gp_kernel")
    def _(x, z, lengthscale, variance, alpha, family):
        return x.new_empty((x.shape[0], x.shape[0] if z is None else z.shape[0]))

    @lib.register_fake("pyro_amd::gp_kernel_bwd")
    def _(x, z, lengthscale, variance, alpha, G, family, want_x, want_z, want_lengthscale, want_variance, want_alpha,
          forced_splits):
        def out(want, like):
            return torch.empty_like(like) if want else x.new_empty((0,))
        want_z = want_z and z is not None
        want_alpha = want_alpha and alpha is not None
        return (out(want_x, x), out(want_z, z if want_z else x), out(want_lengthscale, lengthscale),
                out(want_variance, variance), out(want_alpha, alpha if want_alpha else variance))

    @lib.register_fake("pyro_amd::mixture_fwd_bwd")
    def _(dist, x, a, p0, p1):
        return x.new_empty((a.shape[0], 1 + 3 * a.shape[1]), dtype=torch.float64)

    @lib.register_fake("pyro_amd::lda_factor_indexed")
    def _(words, index, log_theta, log_phi):
        return log_theta.new_empty((words.shape[1],)), torch.empty_like(log_theta), torch.empty_like(log_phi)

    @lib.register_fake("pyro_amd::tall_linear_act")
    def _(G, weight, bias, y_mul, sigmoid_out, transpose_weight):
        return G.new_empty((G.shape[0], weight.shape[0] if transpose_weight else weight.shape[1]))

    @lib.register_fake("pyro_amd::nuts_tree_run_advance")
    def _(z, pe, grad, zq, rq, gq, peq, inv_mass, step, max_tree_depth, use_multinomial, seed, chain_offset, ctl,
          da_state, target_accept, welford, mean_accept, counters, tc, n_done, done_flag, slot2chain, zq_slot,
          accept_prob, stats, workspace):
        return None

    def setup(ctx, inputs, output):
        _, gw, gb, _ws = output
        ctx.save_for_backward(gw, gb)
        ctx.has_b = inputs[3] is not None            # (.., .., w, b, ...) in both schemas
        # only ll is differentiated: without this the engine hands over ZEROS for the other three outputs --
        # the workspace among them, a fill of megabytes per backward pass (9 us of a NUTS round)
        ctx.set_materialize_grads(False)

    def _grads(ctx, g_ll):
        if g_ll is None:
            return None, None
        gw, gb = ctx.saved_tensors
        dw, db = torch.ops.pyro_amd.glm_chain(g_ll, gw, gb)
        return (dw if ctx.needs_input_grad[2] else None,
                db if (ctx.has_b and ctx.needs_input_grad[3]) else None)

    def backward_planes(ctx, g_ll, g_gw, g_gb, g_ws):
        dw, db = _grads(ctx, g_ll)
        # (planes, y, w, b, scale, N, D, format, moments)
        return None, None, dw, db, None, None, None, None, None

    def backward_plain(ctx, g_ll, g_gw, g_gb, g_ws):
        dw, db = _grads(ctx, g_ll)
        # (X, y, w, b, mask, scale)
        return None, None, dw, db, None, None

    lib.register_autograd("pyro_amd::glm_bernoulli_planes", backward_planes, setup_context=setup)
    lib.register_autograd("pyro_amd::glm_bernoulli", backward_plain, setup_context=setup)


def glm_bernoulli_ll(X, y, w, b=None, mask=None, scale=1.0):
    """Per-particle log-likelihood ll[P] of the Bernoulli-logits GLM site through the dispatcher ops
    (same kernel choice as kernels.glm_bernoulli_fwd_bwd: the cached plane image of X once it
    exists, the on-the-fly kernels otherwise); differentiable w.r.t. w[P,D] and b[P]."""
    # sizes and the image lookup are host-side facts about the DATA: taken with the tracer switched
    # off (under torch.jit.trace sizes are traced values, which would also miss the image cache)
    state = torch._C._get_tracing_state()
    torch._C._set_tracing_state(None)
    try:
        N, D = int(X.shape[0]), int(X.shape[1])
        P = int(w.shape[0])
        planes = moments = None
        if (mask is None and D <= kernels.planes_max_d() and P >= kernels._PLANES_MIN_P and N > 0
                and kernels._glm_variant == kernels.GLM_AUTO):
            planes = kernels.glm_planes_of(X)
            if planes is not None:
                moments = kernels.glm_label_moments_of(X, y)
    finally:
        torch._C._set_tracing_state(state)
    y = y.contiguous()
    w = w.contiguous()
    b = b.contiguous() if b is not None else None
    if planes is not None:
        out = torch.ops.pyro_amd.glm_bernoulli_planes(planes, y, w, b, float(scale), N, D,
                                                      kernels._format_of(planes), moments)
    else:
        if mask is not None:
            mask = mask.contiguous()
        out = torch.ops.pyro_amd.glm_bernoulli(X.contiguous(), y, w, b, mask, float(scale))
    keep = kernels._CHAIN["keep"]
    if keep is not None:
        # inside a chained tail the launcher has only RECORDED the finalize phase: the partial records
        # (the op's workspace) and the outputs it writes stay alive until the chain is flushed
        keep.extend(out)
    return out[0]


def adam_step(param, grad, exp_avg, exp_avg_sq, step_dev, lr, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, clip_norm=0.0, lrd=1.0, clipped=False, zero_grad=True):
    """kernels.adam_step through the dispatcher op ``pyro_amd::adam_step`` (in-place on every tensor
    argument): the optimizer update as a graph node of a traced / compiled step."""
    if not available():
        raise RuntimeError("pyro_amd: libpyro_amd_torch.so is not built (python -m pyro_amd.csrc.build)")
    torch.ops.pyro_amd.adam_step(param, grad, exp_avg, exp_avg_sq, step_dev, float(lr), float(betas[0]),
                                 float(betas[1]), float(eps), float(weight_decay), float(clip_norm),
                                 float(lrd), bool(clipped), bool(zero_grad))


# ------------------------------------------------------------------------------------------------------
# autograd Functions as named dispatcher ops
# ------------------------------------------------------------------------------------------------------
ROUTE = {"on": False}
_SPECS = []             # process-local: the non-tensor side of every routed call signature
_SPEC_INDEX = {}
_OPS = {}               # op name -> Function class
_frag = {"lib": None}


class routing:
    """Context manager: ``Function.apply`` of the registered Functions goes through the dispatcher ops
    inside (a tracer switches this on by itself; the context is for tests and torch.compile)."""

    def __enter__(self):
        self._prev = ROUTE["on"]
        ROUTE["on"] = True
        if _WHILE_COMPILING[0] is None:
            import torch._dynamo           # (here, not at import: 0.9 s that only a compiling caller needs)
            _WHILE_COMPILING[0] = torch._dynamo.assume_constant_result(
                lambda name, hkey, n_words: _register_signature(name, hkey, n_words))
        return self

    def __exit__(self, *exc):
        ROUTE["on"] = self._prev
        return False


def _routing_now():
    return ROUTE["on"] or torch._C._get_tracing_state() is not None


class _Slot:
    """Where a tensor argument sat in the call's (nested) argument structure."""
    __slots__ = ("i",)

    def __init__(self, i):
        self.i = i


class _Vol:
    """Where a VOLATILE integer argument sat (a Philox seed, a block offset: new values on every call).  Such
    arguments are not part of a call signature -- the table of signatures would grow by one entry per draw --
    they travel with the call as one int64 host tensor at the end of ``tensors``."""
    __slots__ = ("i", "n")

    def __init__(self, i, n):
        self.i, self.n = i, n          # first word, number of words (None: a plain int)


def _flatten(obj, tensors):
    if isinstance(obj, torch.Tensor):
        tensors.append(obj)
        return _Slot(len(tensors) - 1)
    if isinstance(obj, tuple):
        return tuple(_flatten(o, tensors) for o in obj)
    if isinstance(obj, list):
        return [_flatten(o, tensors) for o in obj]
    if isinstance(obj, dict):
        return {k: _flatten(v, tensors) for k, v in obj.items()}
    return obj


_U64 = (1 << 64) - 1


def _unflatten(obj, tensors, words=None):
    if isinstance(obj, _Slot):
        return tensors[obj.i]
    if isinstance(obj, _Vol):
        if obj.n is None:
            return words[obj.i] & _U64
        return tuple(w & _U64 for w in words[obj.i:obj.i + obj.n])
    if isinstance(obj, tuple):
        return tuple(_unflatten(o, tensors, words) for o in obj)
    if isinstance(obj, list):
        return [_unflatten(o, tensors, words) for o in obj]
    if isinstance(obj, dict):
        return {k: _unflatten(v, tensors, words) for k, v in obj.items()}
    return obj


def _hashable(obj, tensors):
    if isinstance(obj, _Vol):
        return ("V", obj.i, obj.n)
    if isinstance(obj, _Slot):
        t = tensors[obj.i]
        return ("T", tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device), t.requires_grad)
    if isinstance(obj, (tuple, list)):
        return ("tuple" if isinstance(obj, tuple) else "list",) + tuple(_hashable(o, tensors) for o in obj)
    if isinstance(obj, dict):
        return ("dict",) + tuple(sorted((k, _hashable(v, tensors)) for k, v in obj.items()))
    if obj is None or isinstance(obj, (bool, int, float, str, torch.dtype, torch.Size)):
        return obj                     # (spelled out: a compiler inlining this knows these, not ``hash``)
    try:
        hash(obj)
        return obj
    except TypeError:
        return ("id", id(obj))


class _Ctx:
    """What a Function's forward / backward expect of ``ctx``, without the autograd engine behind it."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = needs_input_grad
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, value):
        pass


class _CallSpec:
    def __init__(self, name, fn_cls, structure, top_slots, needs):
        self.name, self.fn_cls, self.structure = name, fn_cls, structure
        self.top_slots = top_slots      # per top-level argument: its tensor index or None
        self.needs = needs              # needs_input_grad as the Function sees it (per argument)
        self.n_out = None               # outputs of the Function (the op returns these + saved tensors)
        self.single = False             # the Function returned one tensor, not a tuple
        self.saved_from = None          # per saved tensor: ("in", j) | ("out", k)
        self.out_meta = None            # (shape, dtype) per op output: the shape function
        self.attrs = {}                 # what forward stored on ctx besides tensors
        self.bwd_none = None            # per tensor input: backward gave no gradient
        self.n_in = 0
        self.n_ret = 0
        self.n_words = 0                # volatile integers riding in the call's last (host) tensor


def _structure_from_key(hk, counter):
    """The argument structure (tensor slots, volatile-integer slots, constants) back from its hashable form:
    tensors were numbered in the order _flatten met them."""
    if isinstance(hk, tuple) and hk:
        tag = hk[0]
        if tag == "T" and len(hk) == 6:
            counter[0] += 1
            return _Slot(counter[0] - 1)
        if tag == "V" and len(hk) == 3:
            return _Vol(hk[1], hk[2])
        if tag == "tuple":
            return tuple(_structure_from_key(o, counter) for o in hk[1:])
        if tag == "list":
            return [_structure_from_key(o, counter) for o in hk[1:]]
        if tag == "dict":
            return {k: _structure_from_key(v, counter) for k, v in hk[1:]}
        if tag == "id":
            raise TypeError("an argument that is neither a tensor nor a constant")
    return hk


def _tensor_entries(hk, out):
    if isinstance(hk, tuple) and hk:
        if hk[0] == "T" and len(hk) == 6:
            out.append(hk)
        elif hk[0] in ("tuple", "list"):
            for o in hk[1:]:
                _tensor_entries(o, out)
        elif hk[0] == "dict":
            for _, v in hk[1:]:
                _tensor_entries(v, out)
    return out


def _register_signature(name, hkey, n_words, structure=None):
    """The table entry of call signature ``hkey`` of op ``name`` (made on first sight).  Everything the entry
    holds follows from the hashable form, so that a compiler can have it made AT RECORDING TIME by a call it
    treats as a constant (``_register_while_compiling``): a table append inside recorded code would only be
    replayed after the recording, too late for the shape functions that run during it."""
    key = (name, hkey)
    sid = _SPEC_INDEX.get(key)
    if sid is None:
        if structure is None:
            structure = _structure_from_key(hkey, [0])
        ents = _tensor_entries(hkey, [])
        top = tuple(a.i if isinstance(a, _Slot) else None for a in structure)
        needs = tuple(isinstance(h, tuple) and len(h) == 6 and h[0] == "T" and bool(h[5]) for h in hkey[1:])
        sp = _CallSpec(name, _OPS[name], structure, top, needs)
        sp.n_in = len(ents)
        sp.in_meta = [(tuple(h[1]), h[3]) for h in ents]       # the shape function of the backward op
        sp.n_words = n_words
        _SPECS.append(sp)
        sid = len(_SPECS) - 1
        _SPEC_INDEX[key] = sid
    return sid


_WHILE_COMPILING = [None]     # _register_signature as a call dynamo evaluates at recording time (made by routing())


def _spec_of(name, fn_cls, args, vol=()):
    tensors = []
    words = []
    if vol:
        args = list(args)
        for i in vol:
            v = args[i]
            if isinstance(v, int):
                args[i] = _Vol(len(words), None)
                words.append(v)
            elif isinstance(v, (tuple, list)) and all(isinstance(x, int) for x in v):
                args[i] = _Vol(len(words), len(v))
                words.extend(v)
    structure = _flatten(tuple(args), tensors)
    hkey = _hashable(structure, tensors)          # (hashable by construction: see _hashable)
    if torch.compiler.is_compiling():
        sid = _WHILE_COMPILING[0](name, hkey, len(words))
    else:
        sid = _register_signature(name, hkey, len(words), structure)
    if words:
        tensors.append(torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in words], dtype=torch.int64))
    return sid, tensors


def _fwd_impl(tensors, spec):
    sp = _SPECS[spec]
    tensors = list(tensors)
    words = tensors.pop().tolist() if sp.n_words else None
    args = _unflatten(sp.structure, tensors, words)
    ctx = _Ctx(sp.needs)
    with torch.no_grad():
        out = sp.fn_cls.forward(ctx, *args)
    single = isinstance(out, torch.Tensor)
    outs = [out] if single else list(out)
    saved = list(ctx.saved_tensors)
    saved_from, extra = [], []
    for s in saved:
        if s is None:
            saved_from.append(("none", 0))
            continue
        hit = next((j for j, t in enumerate(tensors) if t is s), None)
        if hit is not None:
            saved_from.append(("in", hit))          # an input: not returned (an op must not alias its inputs)
            continue
        hit = next((k for k, t in enumerate(outs) if t is s), None)
        if hit is not None:
            saved_from.append(("out", hit))
        else:
            saved_from.append(("out", len(outs) + len(extra)))
            extra.append(s)
    sp.n_out, sp.single, sp.saved_from = len(outs), single, saved_from
    sp.attrs = {k: v for k, v in ctx.__dict__.items() if k not in ("needs_input_grad", "saved_tensors")}
    ret = outs + extra
    # an output that IS an input (or a view of one) would break the op contract: copy it
    ins = {t.untyped_storage().data_ptr() for t in tensors if t.numel() > 0}
    ret = [r.clone() if (r.numel() > 0 and r.untyped_storage().data_ptr() in ins) else r for r in ret]
    sp.out_meta = [(tuple(r.shape), r.dtype) for r in ret]
    sp.n_ret = len(ret)
    return ret


def _fwd_fake(tensors, spec):
    sp = _SPECS[spec]
    if sp.out_meta is None:
        # the shapes of this call signature are not known yet: ONE real evaluation on zero-filled stand-ins
        # of the arguments tells them (outside the fake mode; the kernels' shape rules live in C, there is
        # no second statement of them to keep in step)
        from torch._subclasses.fake_tensor import unset_fake_temporarily
        with unset_fake_temporarily(), torch.no_grad():
            real = [torch.zeros(tuple(t.shape), dtype=t.dtype, device=t.device) for t in tensors]
            _fwd_impl(real, spec)
    proto = tensors[0]
    return [proto.new_empty(shape, dtype=dtype) for shape, dtype in sp.out_meta]


def _bwd_impl(tensors, spec):
    sp = _SPECS[spec]
    grads, saved = list(tensors[:sp.n_out]), list(tensors[sp.n_out:])
    # (a saved None travelled as an empty tensor: back to None)
    saved = [None if kind == "none" else t for (kind, _), t in zip(sp.saved_from, saved)]
    ctx = _Ctx(sp.needs)
    ctx.__dict__.update(sp.attrs)
    ctx.saved_tensors = tuple(saved)
    with torch.no_grad():
        res = sp.fn_cls.backward(ctx, *grads)
    if isinstance(res, torch.Tensor) or res is None:
        res = (res,)
    out, none = [None] * sp.n_in, [True] * sp.n_in
    for pos, j in enumerate(sp.top_slots):
        if j is not None and pos < len(res) and res[pos] is not None:
            out[j], none[j] = res[pos], False
    sp.bwd_none = none
    proto = tensors[0]
    return [proto.new_empty((0,)) if o is None else o for o in out]


def _bwd_fake(tensors, spec):
    sp = _SPECS[spec]
    if sp.bwd_none is None:
        # which inputs get a gradient, before any real backward has run: those the Function was told to
        # differentiate (top-level tensor arguments that required a gradient)
        none = [True] * sp.n_in
        for pos, j in enumerate(sp.top_slots):
            if j is not None and pos < len(sp.needs) and sp.needs[pos]:
                none[j] = False
        sp.bwd_none = none
    proto = tensors[0]
    return [proto.new_empty((0,)) if sp.bwd_none[j] else proto.new_empty(sp.in_meta[j][0], dtype=sp.in_meta[j][1])
            for j in range(sp.n_in)]


def _setup_context(ctx, inputs, output):
    tensors, spec = inputs
    sp = _SPECS[spec]
    saved = []
    for kind, j in sp.saved_from:
        saved.append(None if kind == "none" else (tensors[j] if kind == "in" else output[j]))
    ctx.spec = spec
    ctx.none_saved = [s is None for s in saved]
    ctx.save_for_backward(*[s for s in saved if s is not None])
    ctx.protos = [(o.shape, o.dtype, o.device) for o in output[:sp.n_out]]


def _make_backward(name):
    def backward(ctx, grads):
        sp = _SPECS[ctx.spec]
        gs = []
        for g, (shape, dtype, device) in zip(grads[:sp.n_out], ctx.protos):
            gs.append(torch.zeros(shape, dtype=dtype, device=device) if g is None else g)
        it = iter(ctx.saved_tensors)
        # (a saved None cannot travel in a Tensor[]: an empty tensor stands for it)
        saved = [gs[0].new_empty((0,)) if is_none else next(it) for is_none in ctx.none_saved]
        res = getattr(torch.ops.pyro_amd, name + "_bwd")(gs + saved, ctx.spec)
        # (the host tensor of volatile integers at the end of the inputs has no gradient)
        return [None if sp.bwd_none[j] else res[j] for j in range(sp.n_in)] + [None] * bool(sp.n_words), None
    return backward


def dispatcher_op(fn_name):
    """Class decorator for a ``torch.autograd.Function``: registers ``pyro_amd::<name>`` and
    ``pyro_amd::<name>_bwd`` (see the module docstring) and makes ``apply`` go through them while a
    tracer is recording."""
    def deco(fn_cls):
        if _frag["lib"] is None:
            _frag["lib"] = torch.library.Library("pyro_amd", "FRAGMENT")
        lib = _frag["lib"]
        # the trampoline's op is pyro_amd::fn_<name> (_OPS / the spec table keep the Function's own name); the
        # plain name belongs to the TYPED op of csrc/torch_ops.cpp where one exists
        name = "fn_" + fn_name
        lib.define("%s(Tensor[] tensors, int spec) -> Tensor[]" % name)
        lib.define("%s_bwd(Tensor[] tensors, int spec) -> Tensor[]" % name)
        lib.impl(name, _fwd_impl, "CompositeExplicitAutograd")
        lib.impl(name + "_bwd", _bwd_impl, "CompositeExplicitAutograd")
        torch.library.register_fake("pyro_amd::" + name, _fwd_fake, lib=lib)
        torch.library.register_fake("pyro_amd::" + name + "_bwd", _bwd_fake, lib=lib)
        torch.library.register_autograd("pyro_amd::" + name, _make_backward(name),
                                        setup_context=_setup_context, lib=lib)
        _OPS[fn_name] = fn_cls
        eager_apply = fn_cls.apply
        vol = tuple(getattr(fn_cls, "volatile_args", ()))       # (read here: a compiler inlines ``apply`` below)

        def apply(*args):
            if not _routing_now() or not any(isinstance(a, torch.Tensor) for a in args):
                return eager_apply(*args)
            sid, tensors = _spec_of(fn_name, fn_cls, args, vol)
            out = getattr(torch.ops.pyro_amd, name)(tensors, sid)
            sp = _SPECS[sid]
            return out[0] if sp.single else tuple(out[:sp.n_out])

        fn_cls.apply = staticmethod(apply)
        # the package's call sites use ``invoke``: dynamo special-cases ``apply`` of an autograd.Function
        # (it traces the Function's forward -- ctypes launches it cannot record) but inlines this plain
        # function, which hands the call to the dispatcher op while a tracer / compiler records
        fn_cls.invoke = staticmethod(apply)
        fn_cls.op_name = "pyro_amd::" + name
        return fn_cls
    return deco


def registered_ops():
    """Names of the dispatcher ops of this module (C++ ones once the shim is loaded)."""
    names = ["pyro_amd::fn_" + n for n in _OPS] + ["pyro_amd::fn_" + n + "_bwd" for n in _OPS]
    if available():
        names += ["pyro_amd::" + n for n in ("glm_pack_planes", "glm_bernoulli_planes", "glm_bernoulli",
                                             "glm_chain", "adam_step") + TYPED_OPS]
    return sorted(names)


# the typed C++ ops of csrc/torch_ops.cpp beside the GLM site's (round 6): real argument lists, loadable from C++
TYPED_OPS = ("dist_log_prob_sum", "multi_log_prob_sum", "meanfield_normal_sample", "exp_site", "exp_site_bwd",
             "mvn_tril_sample", "logsumexp_terms", "logchain", "logchain_decode", "mixture_fwd_bwd", "lda_factor_indexed", "tall_linear_act",
             "nuts_tree_run_advance", "gaussian_hmm", "gaussian_hmm_sample", "gaussian_hmm_draw",
             "gaussian_hmm_smooth", "gamma_gaussian_hmm", "linear_hmm_draw", "forecast_scores", "time_transform",
             "gp_kernel", "gp_kernel_bwd")
