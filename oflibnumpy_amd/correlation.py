"""On-demand correlation lookup of two feature tensors in HBM (K18, csrc/ofl_correlation.hip; the definition is in
include/ofl.h): the correlation step of a flow network -- RAFT's multi-level lookup, the local cost volume of PWC-Net --
without the all-pairs volume of (H W)^2 floats.

    corr = DeviceCorrelation.build(fmap1, fmap2, levels=4)        # once per image pair
    for _ in range(iterations):
        feats = corr.lookup(flow, radius=4)                       # (N, 4 * 81, H, W) float32, RAFT's channel order

`build` holds fmap1 and the pyramid of fmap2 channels-last -- a planar tensor is permuted once by K12's permute kernel (one
read and one write of it), level l >= 1 is the float32 2 x 2 mean of level l - 1 -- and `lookup` issues one launch per level on
the library's stream.  Nothing synchronises.
"""
from . import _native as nat
from .args import corr_args
from .batch import DeviceFlowBatch
from .device import DeviceFlow, DeviceTensor
from .kernels import avgpool2_launch, corr_lookup_launch, tensor_permute_launch


def _channels_last(tensor):
    if tensor.layout == 'hwc':
        return tensor.buf
    return tensor_permute_launch(tensor.buf, tensor.dtype, tensor.n, tensor.channels, tensor.h, tensor.w, True)


class DeviceCorrelation:
    """fmap1 and the pyramid of fmap2, channels-last in HBM: `f1` (buffer), `dtype1`, `pyramid` (a list of (buffer, dtype),
    level 0 first), and n, channels, h, w, batched as in DeviceTensor.  Immutable once built."""

    def __init__(self, f1, dtype1, pyramid, n, channels, h, w, batched):
        self.f1, self.dtype1, self.pyramid = f1, dtype1, list(pyramid)
        self.n, self.channels, self.h, self.w, self.batched = n, channels, h, w, batched

    @property
    def levels(self):
        return len(self.pyramid)

    @classmethod
    def build(cls, fmap1, fmap2, levels=4):
        """fmap1, fmap2: DeviceTensors of one logical shape, (C, H, W) or (N, C, H, W), each in either layout and of
        float32, float16 or bfloat16 (the two may differ).  levels: 1 ... 8; level `levels - 1`, of (H >> levels - 1,
        W >> levels - 1) pixels, must not be empty."""
        for name, t in (("fmap1", fmap1), ("fmap2", fmap2)):
            if not isinstance(t, DeviceTensor):
                raise TypeError("Error looking up correlation: {} needs to be a DeviceTensor, got {}".format(name, type(t).__name__))
        if fmap1.shape != fmap2.shape:
            raise ValueError("Error looking up correlation: the feature maps need the same shape, got {} and {}"
                             .format(fmap1.shape, fmap2.shape))
        n, c, h, w = fmap1.n, fmap1.channels, fmap1.h, fmap1.w
        _, levels, _, _, _ = corr_args(1, levels, None, 'xy', nat.QUANT_EXACT, c, (h, w))
        pyramid = [(_channels_last(fmap2), fmap2.dtype)]
        for level in range(1, levels):
            buf, dtype = pyramid[-1]
            pyramid.append((avgpool2_launch(buf, dtype, n, c, h >> (level - 1), w >> (level - 1)), 'float32'))
        return cls(_channels_last(fmap1), fmap1.dtype, pyramid, n, c, h, w, fmap1.batched)

    def lookup(self, flow=None, radius=4, scale=None, order='xy', quant=nat.QUANT_EXACT):
        """The (2 radius + 1)^2 correlation values of every pixel of fmap1 on every level, sampled bilinearly around
        x + flow ('s') or x - flow ('t') scaled to the level, times `scale` (None: float32(1 / sqrt(C))).  flow: a
        DeviceFlow of shape (H, W) -- for one item, or shared by all N --, a DeviceFlowBatch of N, or None (the window
        around the pixel itself); its mask is not read.  order 'xy': channel l (2r + 1)^2 + (ox + r)(2r + 1) + (oy + r),
        what RAFT's CorrBlock produces; 'yx': row-major windows.  quant: nat.QUANT_EXACT, the taps of grid_sample, or
        nat.QUANT_OPENCV, the 1/32-px snap of the warps.  -> a planar float32 DeviceTensor (levels (2r + 1)^2, H, W) or
        (N, ...).  One launch per level; nothing synchronises."""
        radius, _, scale, order, quant = corr_args(radius, self.levels, scale, order, quant, self.channels, (self.h, self.w))
        vecs, shared, sign = None, True, 1
        if flow is not None:
            if isinstance(flow, DeviceFlowBatch):
                if flow.n != self.n:
                    raise ValueError("Error looking up correlation: {} items need a batch of {} fields, got {}".format(self.n, self.n, flow.n))
                shared = False
            elif not isinstance(flow, DeviceFlow):
                raise TypeError("Error looking up correlation: flow needs to be a DeviceFlow, a DeviceFlowBatch or None, got {}"
                                .format(type(flow).__name__))
            if flow.shape != (self.h, self.w):
                raise ValueError("Error looking up correlation: features and flow need the same height and width, got {} and {}"
                                 .format((self.h, self.w), flow.shape))
            vecs, sign = flow.vecs, 1 if flow.ref == 's' else -1
        out = corr_lookup_launch(self.f1, self.dtype1, self.pyramid, self.n, self.channels, self.h, self.w, vecs, shared, sign,
                                 radius, scale, order, quant)
        channels = self.levels * (2 * radius + 1) ** 2
        shape = (self.n, channels, self.h, self.w) if self.batched else (channels, self.h, self.w)
        return DeviceTensor(out, shape, 'float32', 'chw')
