"""Fields at every address a DeviceFlow may have ("Where a field may start"): the bytes of one field inside two
larger host images, one of vectors and one of mask bytes, with poison around them.  No GPU here: test_view_cases_host.py
checks these cases on a CPU, test_gpu_views.py uploads the images and wraps views of them.

A device allocation starts on a 16-byte boundary at least, so an offset into an uploaded image is an address residue: the
vectors at 0 or 8 (mod 16), the mask at 0, 1, 2 or 3 (mod 4).  The poison is what a kernel reads when it takes a pixel
from outside its view, and it is chosen so that this shows: a vector poison pixel is (quiet NaN, 1e30), and the mask
bytes next to the field have the other truth value than the field's own first and last byte."""
import collections

import numpy as np

import test_gpu_matrix
import test_gpu_visualise

F32 = np.float32
GUARD = 64                                       # bytes of poison on either side, at least
VEC_RESIDUES, MASK_RESIDUES = (0, 8), (0, 1, 2, 3)
RESIDUES = [(rv, rm) for rv in VEC_RESIDUES for rm in MASK_RESIDUES]
ODD_RESIDUES = [(8, 1), (8, 3)]                  # what the larger and the degenerate shapes run

# (37, 53): 1961 px, odd, % 4 == 1 -- the batch shape of test_gpu_stream.py; (67, 123): 8241 px, odd, more than one K8
# chunk, one K7 select block and one statistics workgroup; (5, 7): 35 px, % 4 == 3, a three-pixel tail; (1, 3) and (1, 1):
# nothing but head and tail
SHAPES = [(37, 53), (67, 123), (5, 7), (1, 3), (1, 1)]
FULL_SHAPES = [(37, 53), (5, 7)]                 # all eight placements; the other shapes run ODD_RESIDUES

QNAN_BITS, BIG = 0x7fc00000, F32(1e30)

Placement = collections.namedtuple("Placement", "rv rm vimg voff mimg moff shape")


def vec_poison(n_floats):
    """n_floats float32 of alternating quiet NaN and 1e30, starting with the NaN: a poison pixel is (NaN, 1e30)"""
    p = np.empty(n_floats, F32)
    p[0::2] = np.array([QNAN_BITS], np.uint32).view(F32)[0]
    p[1::2] = BIG
    return p


def mask_poison(n, nearest_differs_from, nearest_last):
    """n bytes alternating 0x00 / 0xFF whose byte next to the field (the last one if nearest_last, else the first) has the
    other truth value than the field's byte `nearest_differs_from`"""
    near = 0x00 if nearest_differs_from else 0xFF
    p = np.where(np.arange(n) % 2 == 0, near, near ^ 0xFF).astype(np.uint8)
    return p[::-1].copy() if nearest_last else p


def place(v, m, rv, rm):
    """One Placement: v float32 (H, W, 2) at byte offset voff = rv (mod 16) of vimg, m (H, W) of 0 / 1 at byte offset
    moff = rm (mod 4) of mimg; both images are uint8 arrays whose length is a multiple of 16."""
    v = np.ascontiguousarray(v, F32)
    mb = np.ascontiguousarray(m).astype(np.uint8).reshape(-1)
    h, w = v.shape[:2]
    assert mb.size == h * w and set(np.unique(mb)) <= {0, 1}
    voff = GUARD + rv
    back = GUARD + (-(voff + v.nbytes + GUARD)) % 16
    vimg = np.concatenate([vec_poison(voff // 4), v.reshape(-1), vec_poison(back // 4)]).view(np.uint8)
    moff = GUARD + rm
    back = GUARD + (-(moff + mb.size + GUARD)) % 16
    mimg = np.concatenate([mask_poison(moff, mb[0], True), mb, mask_poison(back, mb[-1], False)])
    return Placement(rv, rm, vimg, voff, mimg, moff, (h, w))


def placements(v, m, residues=RESIDUES):
    """the field's bytes inside two larger host images, for all eight residues (or the given ones)"""
    return [place(v, m, rv, rm) for rv, rm in residues]


def residues_for(shape):
    return RESIDUES if shape in FULL_SHAPES else ODD_RESIDUES


def shape_id(shape):
    """the name of a shape in a test id"""
    return "{}x{}".format(*shape)


def window(p, shift=0):
    """(vecs (H, W, 2) float32, mask (H, W) uint8) as read from the images `shift` pixels behind (+) or in front of (-)
    the field: shift 0 is the field, +-1 takes one poison pixel"""
    h, w = p.shape
    n = h * w
    v = p.vimg[p.voff + 8 * shift: p.voff + 8 * shift + 8 * n].view(F32).reshape(h, w, 2)
    m = p.mimg[p.moff + shift: p.moff + shift + n].reshape(h, w)
    return v, m


# ------------------------------------------------------------------------------ the fields
def random_case(shape, seed=5):
    """seeded standard_normal * 4 with a speckled mask plus a cleared rectangle (test_gpu_visualise) -> (vecs, mask uint8)"""
    v = test_gpu_visualise.random_field(shape[0], shape[1], seed)
    return v, test_gpu_visualise.random_mask(shape[0], shape[1], seed + 1).astype(np.uint8)


def matrix_case(kind, shape, ref):
    """test_gpu_matrix.make_field('holes' / 'noisy') -> (vecs, mask uint8 -- all ones where make_field has none)"""
    vecs, mask, _ = test_gpu_matrix.make_field(kind, shape, ref)
    return vecs, (np.ones(shape, np.uint8) if mask is None else mask.astype(np.uint8))
