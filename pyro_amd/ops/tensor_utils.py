"""Tensor helpers of time-series models (the public names and shape rules of the reference's pyro/ops/tensor_utils.py;
the code is this package's): the orthonormal type-II DCT and the Haar wavelet transform with their inverses,
``next_fast_len``, and the three ``periodic_*`` helpers seasonal models are written with.

Each of the four transforms has two routes, chosen the way ``stats.crps_empirical`` chooses.

Kernel route: device tensors, f32 / f64, ``N <= TIME_TRANSFORM_MAX_STEPS``, ``FUSED_TIME_TRANSFORM = True`` (and, for
the DCT in f64 over 1024 steps, at most ``DCT_F64_LONG_MAX_SERIES`` series: a measured crossover).  ONE
launch of pa_time_transform (csrc/time_transform.hip) through an autograd Function whose backward is the inverse
kernel -- the transforms are orthonormal, so the adjoint of each is its inverse -- one more launch, no saved tensor.
A transform along ``dim != -1`` goes to the kernel as [outer, N, inner] without a transpose.

Torch route: everything else (CPU tensors, other dtypes, longer N, the switch off, a double backward), written in
torch operators from the definitions (an FFT of the even-odd permuted signal for the DCT, the level loop for Haar) and
differentiable by autograd.

An empty tensor makes no launch on either route.
"""
import math

import torch

from .torch_library import dispatcher_op as _dispatcher_op

FUSED_TIME_TRANSFORM = True       # device f32 / f64 tensors, N <= TIME_TRANSFORM_MAX_STEPS: pa_time_transform
TIME_TRANSFORM_MAX_STEPS = 2048   # (kernels.TIME_TRANSFORM_MAX_STEPS, csrc/time_transform.hip TT_MAX_STEPS)
# Routing by measurement (tools/bench_time_transform.py, forward plus backward of idct, MI355X): the DCT kernel does
# O(N^2) work per series and takes strips of only 2 series in f64 over 1024 steps.  There it won at 4 series
# ([1, 2048, 4]: 202-226 us against the torch route's 413-535) and lost at 256 ([64, 2048, 4]: 536-568 us against
# 443-543); the crossover by linear interpolation is near 190 series.  Every other measured shape the kernel won.
DCT_F64_LONG_STEPS = 1024
DCT_F64_LONG_MAX_SERIES = 128
_DCT, _IDCT, _HAAR, _IHAAR = 0, 1, 2, 3
_ROOT_HALF = math.sqrt(0.5)


# ---- the kernel route --------------------------------------------------------------------------------------------
@_dispatcher_op("time_transform")
class _TimeTransform(torch.autograd.Function):
    """y = op(x) along ``dim``, ONE launch (pa_time_transform); the gradient is the inverse op of the incoming
    gradient, one more launch, nothing saved."""

    @staticmethod
    def forward(ctx, x, op, dim):
        from .. import kernels
        ctx.op, ctx.dim = op, dim
        return kernels.time_transform(x, op, dim)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import kernels
        return kernels.time_transform(g, kernels.TIME_TRANSFORM_ADJOINT[ctx.op], ctx.dim), None, None


def _fused(x, op, dim):
    from .. import kernels
    if not (FUSED_TIME_TRANSFORM and kernels.on_device(x) and x.dtype in (torch.float32, torch.float64)):
        return False
    n = x.shape[dim]
    if n > TIME_TRANSFORM_MAX_STEPS or x.numel() == 0:
        return False
    if (op in (_DCT, _IDCT) and x.dtype == torch.float64 and n > DCT_F64_LONG_STEPS
            and x.numel() // n > DCT_F64_LONG_MAX_SERIES):
        return False
    return True


def _transform(x, op, dim):
    if x.dim() == 0:
        raise ValueError("a time transform needs a tensor with at least one dim")
    if dim >= 0:
        dim -= x.dim()
    if not -x.dim() <= dim:
        raise IndexError("dim {} of a {}-d tensor".format(dim, x.dim()))
    if x.numel() == 0:
        return x.clone()
    if _fused(x, op, dim):
        return _TimeTransform.invoke(x, op, dim)
    if dim != -1:
        return _TORCH_ROUTE[op](x.transpose(dim, -1)).transpose(dim, -1)
    return _TORCH_ROUTE[op](x)


# ---- the torch route ---------------------------------------------------------------------------------------------
def _dct_scales(x, n):
    scale = x.new_full((n,), math.sqrt(2.0 / n))
    scale[0] = math.sqrt(1.0 / n)
    return scale


def _quarter_phases(x, n):
    """exp(-i pi k / 2N), k = 0..N-1, in x's precision."""
    k = torch.arange(n, dtype=x.dtype, device=x.device) * (math.pi / (2 * n))
    return torch.complex(k.cos(), -k.sin())


def _dct_torch(x):
    # Makhoul 1980: with v = (x_0, x_2, ..., x_3, x_1), sum_n x_n cos(pi (2n + 1) k / 2N) = Re(e^{-i pi k / 2N} V_k)
    n = x.size(-1)
    v = torch.cat([x[..., 0::2], x[..., 1::2].flip(-1)], dim=-1)
    spectrum = torch.fft.fft(v, dim=-1)
    return (spectrum * _quarter_phases(x, n)).real * _dct_scales(x, n)


def _idct_torch(y):
    # the steps of _dct_torch undone: V_k = e^{i pi k / 2N} (c_k - i c_{N-k}) with c = y / scale, c_N = 0
    n = y.size(-1)
    c = y / _dct_scales(y, n)
    mirrored = torch.cat([c.new_zeros(c.shape[:-1] + (1,)), c[..., 1:].flip(-1)], dim=-1)
    spectrum = torch.complex(c, -mirrored) * _quarter_phases(y, n).conj()
    v = torch.fft.ifft(spectrum, dim=-1).real
    half = (n + 1) // 2
    x = torch.empty_like(v)
    x[..., 0::2] = v[..., :half]
    x[..., 1::2] = v[..., half:].flip(-1)
    return x


def _haar_torch(x):
    # level by level: the pairs of the current low band [0, len) -> (lo, hi); hi and an odd tail are final
    pieces, low = [], x
    while True:
        n = low.size(-1) // 2
        even, odd, tail = low[..., 0:2 * n:2], low[..., 1:2 * n:2], low[..., 2 * n:]
        pieces = [(even - odd) * _ROOT_HALF, tail] + pieces
        low = (even + odd) * _ROOT_HALF
        if n < 2:
            return torch.cat([low] + pieces, dim=-1)


def _inverse_haar_torch(y):
    lengths = [y.size(-1)]
    while lengths[-1] // 2 >= 2:
        lengths.append(lengths[-1] // 2)
    low = y[..., :lengths[-1] // 2]
    for length in reversed(lengths):
        n = length // 2
        hi, tail = y[..., n:2 * n], y[..., 2 * n:length]
        pairs = torch.stack([(low + hi) * _ROOT_HALF, (low - hi) * _ROOT_HALF], dim=-1)
        low = torch.cat([pairs.reshape(pairs.shape[:-2] + (2 * n,)), tail], dim=-1)
    return low


_TORCH_ROUTE = {_DCT: _dct_torch, _IDCT: _idct_torch, _HAAR: _haar_torch, _IHAAR: _inverse_haar_torch}


# ---- the public functions ----------------------------------------------------------------------------------------
def dct(x, dim=-1):
    """The discrete cosine transform of type II along ``dim``, scaled to be orthonormal (scipy.fftpack.dct with
    norm="ortho"); the inverse of :func:`idct`."""
    return _transform(x, _DCT, dim)


def idct(x, dim=-1):
    """The inverse of :func:`dct` (scipy.fftpack.idct with norm="ortho")."""
    return _transform(x, _IDCT, dim)


def haar_transform(x, dim=-1):
    """The discrete Haar wavelet transform along ``dim`` (the reference's function has the last dim only), any length: per level, with n = len // 2, the output
    is [lo(n), hi(n), tail(len - 2n)], hi = (even - odd) / sqrt 2, and lo = (even + odd) / sqrt 2 is transformed
    further while n >= 2.  Length 0 or 1 is the identity.  The inverse of :func:`inverse_haar_transform`."""
    return _transform(x, _HAAR, dim)


def inverse_haar_transform(x, dim=-1):
    """The inverse of :func:`haar_transform`."""
    return _transform(x, _IHAAR, dim)


_FAST_LENGTHS = {}


def next_fast_len(size):
    """The smallest n >= ``size`` with no prime factor other than 2, 3 and 5 (scipy.fftpack.next_fast_len)."""
    assert isinstance(size, int) and size > 0
    found = _FAST_LENGTHS.get(size)
    if found is None:
        found = size
        while True:
            rest = found
            for prime in (2, 3, 5):
                while rest % prime == 0:
                    rest //= prime
            if rest == 1:
                break
            found += 1
        _FAST_LENGTHS[size] = found
    return found


def periodic_repeat(tensor, size, dim):
    """``tensor`` repeated along ``dim`` (period = its size there) and cut to ``size``: static seasonality, and how
    the value drawn for one subsample initialises the parameter of the FULL plate in the autoguides."""
    assert isinstance(size, int) and size >= 0
    assert isinstance(dim, int)
    if dim >= 0:
        dim -= tensor.dim()
    period = tensor.size(dim)
    repeats = [1] * tensor.dim()
    repeats[dim] = -(-size // period)
    return tensor.repeat(*repeats).narrow(dim, 0, size)


def periodic_cumsum(tensor, period, dim):
    """The cumulative sum along ``dim`` within each residue class modulo ``period``: result[t] = tensor[t] +
    result[t - period] (drifting seasonality)."""
    assert isinstance(period, int) and period > 0
    assert isinstance(dim, int)
    if dim >= 0:
        dim -= tensor.dim()
    size = tensor.size(dim)
    cycles = -(-size // period)
    padding = cycles * period - size
    if padding:
        tensor = torch.cat([tensor, tensor.new_zeros(tensor.shape[:dim] + (padding,) + tensor.shape[tensor.dim() + dim + 1:])],
                           dim)
    folded = tensor.reshape(tensor.shape[:dim] + (cycles, period) + tensor.shape[tensor.dim() + dim + 1:])
    return folded.cumsum(dim - 1).reshape(tensor.shape).narrow(dim, 0, size)


def periodic_features(duration, max_period=None, min_period=None, **options):
    """Cosine and sine features of the periods ``max_period / j``, j = 1, 2, ... down to ``min_period`` (exclusive;
    default 2, the Nyquist limit; ``max_period`` defaults to ``duration``): a tensor of shape
    (duration, 2 * ceil(max_period / min_period) - 2) with values in [-1, 1].  ``options``: dtype, device."""
    assert isinstance(duration, int) and duration >= 0
    max_period = duration if max_period is None else max_period
    min_period = 2 if min_period is None else min_period
    assert 2 <= min_period, "min_period is below the Nyquist limit"
    assert min_period <= max_period
    t = torch.arange(float(duration), **options).reshape(-1, 1, 1)
    phase = torch.tensor([0.0, math.pi / 2], **options).reshape(2, 1)
    freq = torch.arange(1, max_period / min_period, **options) * (2 * math.pi / max_period)
    return (freq * t + phase).cos().reshape(duration, -1).contiguous()
