"""The cases of the forecast-score tests (host and device) and of the generator of tests/golden/forecast.npz: pred
[S, M] samples against truth [M], built in float64 from a seed that depends on the case alone, never modified.

The bounds are the ones the tests share:
  float64: |mean - ref|, |crps - ref| <= S * 2^-52 * (1 + A), A the largest finite magnitude of the case -- the
           rounding bound of an S-term sum of terms of magnitude up to A;
  float32: the error against the float64 torch formula is at most four times the error of the float32 torch formula on
           the CPU, with floor 4 * 2^-23 * (1 + A);
  median:  bit-equal to torch's median(0).values.
"""
import os
import zlib

import numpy as np
import torch

SAMPLES = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 1000, 1024)
OVER = 1025                                   # takes the torch route
STRIPS = (32, 16)                             # the strip widths the kernel instantiates
COLUMNS = tuple(sorted({1} | {m for c in STRIPS for m in (c - 1, c, c + 1, 3 * c + 5)}))
KINDS = ("random", "equal", "ties", "sorted", "reversed", "below", "above", "hit", "shifted", "nan_sample",
         "nan_truth", "inf_sample", "transposed", "lead_ones")
# (kind, S, M) whose reference results are in the fixture
GOLDEN = (("random", 1, 17), ("random", 2, 33), ("random", 3, 16), ("random", 64, 31), ("random", 129, 15),
          ("random", 1000, 1), ("random", 1024, 1), ("ties", 65, 32), ("equal", 4, 53), ("hit", 127, 17),
          ("shifted", 128, 33), ("reversed", 63, 101), ("below", 3, 1))
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forecast.npz")
_CACHE = {}


def golden(prefix):
    """{name: read-only numpy array} of the fixture's entries under ``prefix``/."""
    if not _CACHE:
        with np.load(_PATH) as z:
            for key in z.files:
                a = z[key]
                a.setflags(write=False)
                _CACHE[key] = a
    return {k[len(prefix) + 1:]: v for k, v in _CACHE.items() if k.startswith(prefix + "/")}


def bad_column(M):
    """The column that carries the NaN / inf of a case."""
    return (2 * M) // 3


def make(kind, S, M):
    """(pred, truth) of a case as float64 CPU tensors.  ``pred`` is [S, M] except for "lead_ones", where it is
    (S, 1, 1) + truth.shape with truth [M]; "transposed" returns a non-contiguous view of an [M, S] tensor."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (kind, S, M)).encode()))
    p = rng.standard_normal((S, M))
    y = rng.standard_normal(M)
    if kind == "equal":
        p = np.broadcast_to(rng.standard_normal(M), (S, M)).copy()
    elif kind == "ties":
        p = np.where(p > 0, 0.75, -0.25)
    elif kind == "sorted":
        p = np.sort(p, axis=0)
    elif kind == "reversed":
        p = np.sort(p, axis=0)[::-1].copy()
    elif kind == "below":
        y = p.min(axis=0) - 1.0 - rng.random(M)
    elif kind == "above":
        y = p.max(axis=0) + 1.0 + rng.random(M)
    elif kind == "hit":
        y = p[rng.integers(0, S, M), np.arange(M)].copy()
    elif kind == "shifted":
        p, y = p + 1e3, y + 1e3
    elif kind == "nan_sample":
        p[S // 2, bad_column(M)] = np.nan
    elif kind == "nan_truth":
        y[bad_column(M)] = np.nan
    elif kind == "inf_sample":
        p[S // 2, bad_column(M)] = np.inf
    pred, truth = torch.tensor(p), torch.tensor(y)
    if kind == "transposed":
        pred = pred.t().contiguous().t()
        assert not pred.is_contiguous() or min(S, M) == 1
    elif kind == "lead_ones":
        pred = pred.reshape(S, 1, 1, M)
    return pred, truth


def torch_formula(pred, truth):
    """(mean, median, crps) by the reference's formulas in torch ops, in the dtype and on the device of ``pred``
    [S, M]; a NaN truth makes the column NaN in all three, as the kernel's contract has it."""
    S = pred.shape[0]
    mean, median = pred.mean(0), pred.median(0).values
    if S == 1:
        crps = (pred[0] - truth).abs()
    else:
        srt = pred.sort(dim=0).values
        diff = srt[1:] - srt[:-1]
        i = torch.arange(1, S, dtype=pred.dtype, device=pred.device)
        crps = (srt - truth).abs().mean(0) - (diff * (i * (S - i)).unsqueeze(-1)).sum(0) / S ** 2
    nan = torch.isnan(truth)
    return mean.masked_fill(nan, float("nan")), median.masked_fill(nan, float("nan")), crps


def magnitude(pred, truth):
    """A: the largest finite magnitude in the case."""
    vals = torch.cat([pred.reshape(-1), truth.reshape(-1)]).double()
    vals = vals[torch.isfinite(vals)]
    return float(vals.abs().max()) if vals.numel() else 0.0


def bound64(S, A):
    return S * 2.0 ** -52 * (1.0 + A)


def floor32(A):
    return 4 * 2.0 ** -23 * (1.0 + A)


def same_nonfinite(got, want):
    """Non-finite entries agree in kind (NaN with NaN, an infinity with the same infinity)."""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    return bool((torch.isfinite(got) == fin).all() and (torch.isnan(got) == torch.isnan(want)).all()
                and (got[~fin & ~torch.isnan(want)] == want[~fin & ~torch.isnan(want)]).all())


def max_err(got, want):
    """Largest |got - want| over the entries where ``want`` is finite (0 if none)."""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    return float((got[fin] - want[fin]).abs().max()) if bool(fin.any()) else 0.0
