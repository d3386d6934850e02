"""``dist.transforms``: everything of torch.distributions.transforms, plus the two unit-Jacobian transforms along a time
axis (the public interface of the reference's pyro/distributions/transforms/{discrete_cosine,haar}.py; the code is
this package's).  They sit on ``pyro_amd.ops.tensor_utils``, so device f32 / f64 tensors of up to
``tensor_utils.TIME_TRANSFORM_MAX_STEPS`` steps take one launch of pa_time_transform per direction, also along
``dim != -1`` (no transpose is made), and one more for a gradient."""
import torch
from torch.distributions import constraints
from torch.distributions import transforms as _torch_transforms
from torch.distributions.transforms import Transform

from ..ops import tensor_utils

globals().update({_name: getattr(_torch_transforms, _name) for _name in dir(_torch_transforms)
                  if not _name.startswith("__")})
__all__ = list(_torch_transforms.__all__) + ["DiscreteCosineTransform", "HaarTransform"]


class _UnitJacobianTimeTransform(Transform):
    """An orthonormal map along the absolute, negative dim ``dim``: the dims from ``dim`` on form one event."""
    bijective = True

    def __init__(self, dim, cache_size):
        assert isinstance(dim, int) and dim < 0, "dim counts from the right and is negative"
        self.dim = dim
        super().__init__(cache_size=cache_size)

    @constraints.dependent_property(is_discrete=False)
    def domain(self):
        return constraints.independent(constraints.real, -self.dim)

    @constraints.dependent_property(is_discrete=False)
    def codomain(self):
        return constraints.independent(constraints.real, -self.dim)

    def log_abs_det_jacobian(self, x, y):
        return x.new_zeros(x.shape[:self.dim])

    def forward_shape(self, shape):
        if len(shape) < -self.dim:
            raise ValueError("Too few dimensions on input")
        return shape

    inverse_shape = forward_shape


class DiscreteCosineTransform(_UnitJacobianTimeTransform):
    """The orthonormal type-II DCT along ``dim`` (tensor_utils.dct / idct).  ``smooth``: frequency k + 1/2 is weighted
    by (k + 1/2) ** smooth, normalised to unit geometric mean so that the Jacobian stays 1: 0 takes white noise to
    white noise, 1 Brownian noise to white noise, -1 violet noise to white noise; any real number is allowed.  The
    weights are a torch multiply beside the kernel."""

    def __init__(self, dim=-1, smooth=0.0, cache_size=0):
        self.smooth = float(smooth)
        self._weights = None
        super().__init__(dim, cache_size)

    def __hash__(self):
        return hash((type(self), self.dim, self.smooth))

    def __eq__(self, other):
        return type(self) == type(other) and self.dim == other.dim and self.smooth == other.smooth

    @torch.no_grad()
    def _weight(self, y):
        size = y.size(self.dim)
        w = self._weights
        if w is None or w.numel() != size or w.dtype != y.dtype or w.device != y.device:
            freq = torch.linspace(0.5, size - 0.5, size, dtype=y.dtype, device=y.device)
            w = freq.pow(self.smooth)
            w = w / w.log().mean().exp()
            self._weights = w = w.reshape((size,) + (1,) * (-1 - self.dim))
        return w

    def _call(self, x):
        y = tensor_utils.dct(x, self.dim)
        return y * self._weight(y) if self.smooth else y

    def _inverse(self, y):
        if self.smooth:
            y = y / self._weight(y)
        return tensor_utils.idct(y, self.dim)

    def with_cache(self, cache_size=1):
        if self._cache_size == cache_size:
            return self
        return DiscreteCosineTransform(self.dim, self.smooth, cache_size=cache_size)


class HaarTransform(_UnitJacobianTimeTransform):
    """The orthonormal Haar wavelet transform along ``dim`` (tensor_utils.haar_transform and its inverse); for a
    length that is no power of two, a block-structured one whose blocks halve from left to right.  ``flip``: reverse
    time first."""

    def __init__(self, dim=-1, flip=False, cache_size=0):
        self.flip = flip
        super().__init__(dim, cache_size)

    def __hash__(self):
        return hash((type(self), self.dim, self.flip))

    def __eq__(self, other):
        return type(self) == type(other) and self.dim == other.dim and self.flip == other.flip

    def _call(self, x):
        if self.flip:
            x = x.flip(self.dim)
        return tensor_utils.haar_transform(x, self.dim)

    def _inverse(self, y):
        x = tensor_utils.inverse_haar_transform(y, self.dim)
        return x.flip(self.dim) if self.flip else x

    def with_cache(self, cache_size=1):
        if self._cache_size == cache_size:
            return self
        return HaarTransform(self.dim, flip=self.flip, cache_size=cache_size)
