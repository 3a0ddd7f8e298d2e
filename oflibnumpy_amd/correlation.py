"""On-demand correlation lookup of two feature tensors in HBM (K18, csrc/ofl_correlation.hip; the definition is in
include/ofl.h): the correlation step of a flow network -- RAFT's multi-level lookup, the local cost volume of PWC-Net --
without the all-pairs volume of (H W)^2 floats.

    corr = DeviceCorrelation.build(fmap1, fmap2, levels=4)        # once per image pair
    for _ in range(iterations):
        feats = corr.lookup(flow, radius=4)                       # (N, 4 * 81, H, W) float32, RAFT's channel order

`build` holds fmap1 and the pyramid of fmap2 channels-last -- a planar tensor is permuted once by K12's permute kernel (one
read and one write of it), level l >= 1 is the float32 2 x 2 mean of level l - 1 -- and `lookup` issues one launch per level on
the library's stream.  Nothing synchronises.

The same two buffers answer "where is the best match anywhere?" (K19, csrc/ofl_match.hip): `corr.match()` dots every pixel of
fmap1 with every pixel of fmap2 on the matrix cores, runs the softmax over all H W candidates and returns the expected
displacement as a DeviceFlow -- the first flow of a GMFlow-style matcher -- again without the all-pairs volume.
"""
from . import _native as nat
from .args import corr_args, match_args, optional_bool
from .batch import DeviceFlowBatch
from .device import DeviceFlow, DeviceTensor
from .kernels import avgpool2_launch, corr_lookup_launch, match_launch, tensor_permute_launch


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

    def match(self, ref='s', scale=None, reverse=False, min_confidence=None, return_confidence=False, return_index=False):
        """The global match of every pixel of fmap1 among ALL pixels of fmap2 (level 0): the softmax over the H W dot
        products times `scale` (None: float32(1 / sqrt(C))), the expected coordinate minus the pixel's own as the flow --
        with ref 's' pixel + flow is the match, 't' is its exact negation.  reverse=True matches the pixels of fmap2 into
        fmap1 (the two buffers swapped): the backward field for DeviceFlow.consistency.  The mask is set where the
        confidence, the softmax probability of the best candidate, is at least `min_confidence` (None: 0, every pixel).
        Both feature maps need one dtype.  -> a DeviceFlow, or a DeviceFlowBatch for (N, C, H, W); with return_confidence /
        return_index a tuple that also holds the float32 confidence [N][H][W] and the int32 row-major index of the best
        candidate [N][H][W] as DeviceBuffers.  One launch; nothing synchronises."""
        from .utils import get_valid_ref
        ref = get_valid_ref(ref)
        flags = [optional_bool(v, False, "Error matching features: {} needs to be a boolean".format(name))
                 for name, v in (("reverse", reverse), ("return_confidence", return_confidence), ("return_index", return_index))]
        f2, dtype2 = self.pyramid[0]
        scale, min_conf = match_args(scale, min_confidence, self.channels, self.dtype1, dtype2)
        a, b = (f2, self.f1) if flags[0] else (self.f1, f2)
        vecs, mask, conf, index = match_launch(a, b, self.dtype1, self.n, self.channels, self.h, self.w, scale,
                                               1 if ref == 's' else -1, min_conf, flags[1], flags[2])
        shape = (self.h, self.w)
        flow = DeviceFlowBatch.wrap(self.n, shape, ref, vecs, mask) if self.batched else DeviceFlow(vecs, mask, shape, ref)
        extra = tuple(x for x, wanted in ((conf, flags[1]), (index, flags[2])) if wanted)
        return (flow,) + extra if extra else flow
