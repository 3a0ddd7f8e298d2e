"""CPU suite: the host half of the median filter (K16) -- args.median_args, the mask validators, the ctypes table, the argument
checks of Flow.median and median_flow -- and the NumPy restatement tests/median_ref.py that test_gpu_median.py compares the
kernel with: against SciPy's median_filter in the interior of all-valid finite fields (the one independent yardstick; SciPy
knows no masks), against a plain sorted() loop on masked fields with special values, and the key as an order.  The sorting
network of csrc/ofl_median_net.h is compiled for the host and checked against std::sort."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
from scipy import ndimage

import oflibnumpy_amd as of
from oflibnumpy_amd import args, build_native as bn, _native as nat
import median_ref as M


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("ksize", M.KSIZES)
def test_restatement_equals_scipys_median_filter_in_the_interior(ksize):
    shape, r = (37, 53), ksize // 2
    v = M.vectors(shape, specials=False)
    out, out_mask, n = M.median(v, np.ones(shape, np.uint8), ksize)
    assert out_mask.all() and (n[r:-r, r:-r] == ksize * ksize).all() and n[0, 0] == (r + 1) ** 2
    for c in (0, 1):
        want = ndimage.median_filter(v[..., c], size=ksize)
        assert np.array_equal(out[r:-r, r:-r, c], want[r:-r, r:-r])


def _py_key(f):
    b = struct.unpack("<I", struct.pack("<f", f))[0]
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


@pytest.mark.parametrize("ksize", M.KSIZES)
@pytest.mark.parametrize("name", ["random50", "random5", "checker", "all"])
def test_restatement_equals_a_sorted_loop(ksize, name):
    shape, r = (37, 53), ksize // 2
    h, w = shape
    rng = np.random.default_rng(3)
    v, m = M.vectors(shape), M.mask(name, shape)
    valid = (rng.random(shape) < 0.8).astype(np.uint8) if name == "random50" else None
    only = (rng.random(shape) < 0.5).astype(np.uint8) if name != "all" else None
    min_count = {"random50": 3, "random5": 1, "checker": ksize * ksize // 2, "all": ksize * ksize}[name]
    out, out_mask, n = M.median(v, m, ksize, valid, only, min_count)
    words, in_words = out.view(np.uint32), v.view(np.uint32)
    mem = m if valid is None else m & valid
    pixels = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (r, r), (h // 2, w // 2)]
    pixels += [(int(rng.integers(h)), int(rng.integers(w))) for _ in range(150)]
    for y, x in pixels:
        q = [(qy, qx) for qy in range(max(0, y - r), min(h, y + r + 1)) for qx in range(max(0, x - r), min(w, x + r + 1)) if mem[qy, qx]]
        assert n[y, x] == len(q)
        target = True if only is None else bool(only[y, x])
        ok = target and len(q) >= min_count
        for c in (0, 1):
            if ok:
                ranked = sorted((_py_key(v[qy, qx, c]), int(in_words[qy, qx, c])) for qy, qx in q)
                assert int(words[y, x, c]) == ranked[(len(q) - 1) >> 1][1], (y, x, c)
            else:
                assert words[y, x, c] == in_words[y, x, c]
        assert out_mask[y, x] == ((1 if ok else 0) if target else (1 if m[y, x] else 0))
    if name == "random5":
        assert (n == 0).mean() >= (1 / 3 if ksize == 3 else 0)
    if name == "all":                                                      # min_count = k^2: the border loses its mask
        assert not out_mask[0].any() and out_mask[r:-r, r:-r].all() and out[0].tobytes() == v[0].tobytes()


def test_key_is_a_bijection_and_an_order():
    f = np.array([-np.inf, -3.0e38, -1.0, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 1.0, 2.0, 3.0e38, np.inf], np.float32)
    k = M.key(f)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()          # -0.0 < +0.0 included
    assert M.unkey(k).tobytes() == f.tobytes()
    assert [int(x) for x in k] == [_py_key(float(x)) for x in f]
    words = np.concatenate([M.SPECIAL, np.random.default_rng(1).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
    k = M.key(words.view(np.float32))
    assert M.unkey(k).view(np.uint32).tolist() == words.tolist() and len(set(k.tolist())) == len(set(words.tolist()))
    # NaNs sort beyond the infinities, by sign
    nan_pos, nan_neg = M.key(np.array([0x7FC00000], np.uint32).view(np.float32))[0], M.key(np.array([0xFFC00000], np.uint32).view(np.float32))[0]
    assert nan_neg < M.key(np.float32(-np.inf).reshape(1))[0] and nan_pos > M.key(np.float32(np.inf).reshape(1))[0]


def test_lower_median_and_despeckle_by_hand():
    v = np.zeros((1, 4, 2), np.float32)
    v[0, :, 0] = [4, 1, 3, 2]
    v[0, :, 1] = [-0.0, 0.0, -0.0, 0.0]
    out, out_mask, n = M.median(v, np.ones((1, 4), np.uint8), 3)
    assert n.tolist() == [[2, 3, 3, 2]] and out[0, :, 0].tolist() == [1, 3, 2, 2]              # even counts: the lower one
    assert np.signbit(out[0, :, 1]).tolist() == [True, True, False, True]                       # -0.0 < +0.0: {-0, +0, -0} -> -0, {+0, -0, +0} -> +0
    # a pixel valid excludes takes its neighbours' median and becomes valid; an isolated pixel is despeckled
    m, valid = np.array([[1, 1, 1, 0, 0, 0, 1]], np.uint8), np.array([[1, 0, 1, 1, 1, 1, 1]], np.uint8)
    v = np.zeros((1, 7, 2), np.float32)
    v[0, :, 0] = [5, 99, 7, 1, 1, 1, 8]
    out, out_mask, n = M.median(v, m, 3, valid, None, 2)
    assert n.tolist() == [[1, 2, 1, 1, 0, 1, 1]] and out_mask.tolist() == [[0, 1, 0, 0, 0, 0, 0]]
    assert out[0, :, 0].tolist() == [5, 5, 7, 1, 1, 1, 8]
    # only: the others keep vector and mask
    out, out_mask, _ = M.median(v, m, 3, valid, np.array([[0, 1, 0, 0, 0, 0, 0]], np.uint8), 2)
    assert out_mask.tolist() == [[1, 1, 1, 0, 0, 0, 1]] and out[0, :, 0].tolist() == [5, 5, 7, 1, 1, 1, 8]


def test_sorting_network_sorts():
    """csrc/ofl_median_net.h on the host: exhaustive 0-1 inputs for 9 wires (the 0-1 principle), random words, few distinct
    values and 0-1 patterns for 25 and 49 wires against std::sort"""
    src = r'''
#include "ofl_median_net.h"
#include <algorithm>
#include <stdio.h>
template <int N> bool check() {
    uint32_t a[N], b[N], s = 12345u + N;
    for (int it = 0; it < 30000; ++it) {
        for (int i = 0; i < N; ++i) { s = s * 1664525u + 1013904223u; const uint32_t r = s >> 8; a[i] = it % 3 == 0 ? (r & 1) : it % 3 == 1 ? r % 5 : s; }
        std::copy(a, a + N, b); std::sort(b, b + N);
        ofl::net_sort<N>(a);
        if (!std::equal(a, a + N, b)) return false;
    }
    return true;
}
int main() {
    for (unsigned m = 0; m < 512; ++m) {
        uint32_t a[9];
        for (int i = 0; i < 9; ++i) a[i] = (m >> i) & 1;
        ofl::net_sort<9>(a);
        for (int i = 1; i < 9; ++i) if (a[i - 1] > a[i]) return 1;
    }
    if (!check<9>() || !check<25>() || !check<49>()) return 2;
    puts("ok");
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "net.cpp")
        open(c, "w").write(src)
        exe = os.path.join(d, "net")
        r = subprocess.run(["c++", "-std=c++17", "-O1", "-I", bn.CSRC, c, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == "ok"


# ---------------------------------------------------------------------------------------------- median_args, the validators
def test_median_args_values():
    assert args.median_args() == (5, 1) and args.median_args(3) == (3, 1) and args.median_args(7, None) == (7, 1)
    assert args.median_args(np.int64(3), np.int32(9)) == (3, 9) and args.median_args(7, 49) == (7, 49) and args.median_args(5, 13) == (5, 13)
    assert all(type(x) is int for x in args.median_args(np.int64(3), np.int32(9)))


@pytest.mark.parametrize("bad", [True, np.True_, 3.0, np.float32(5), "3", None, [3], (5,)])
def test_median_args_ksize_type_errors(bad):
    with pytest.raises(TypeError, match="Error filtering flow"):
        args.median_args(bad)


@pytest.mark.parametrize("bad", [4, 6, 2, 1, 0, -3, 9, 8])
def test_median_args_ksize_value_errors(bad):
    with pytest.raises(ValueError, match="Error filtering flow"):
        args.median_args(bad)


def test_median_args_min_count_errors():
    for ksize in M.KSIZES:
        for bad in (0, ksize * ksize + 1, -1):
            with pytest.raises(ValueError, match="Error filtering flow"):
                args.median_args(ksize, bad)
    for bad in (True, 2.0, "2", [2]):
        with pytest.raises(TypeError, match="Error filtering flow"):
            args.median_args(3, bad)


@pytest.mark.parametrize("name", ["valid", "only"])
def test_median_mask_array(name):
    a = args.mask_array_arg(np.ones((4, 6), bool), (4, 6), "Error filtering flow: ", name)
    assert a.dtype == np.uint8 and a.shape == (4, 6) and a.flags.c_contiguous and a.all()
    assert args.mask_array_arg(np.zeros((4, 6), np.uint8), (4, 6, 2), "Error filtering flow: ", name).dtype == np.uint8
    with pytest.raises(ValueError, match=r"{}.*\(4, 5\).*\(4, 6\)".format(name)):
        args.mask_array_arg(np.ones((4, 5), bool), (4, 6), "Error filtering flow: ", name)
    with pytest.raises(ValueError, match=name):
        args.mask_array_arg(np.ones((4, 6, 1), bool), (4, 6), "Error filtering flow: ", name)
    with pytest.raises(TypeError, match=name + ".*float32"):
        args.mask_array_arg(np.ones((4, 6), np.float32), (4, 6), "Error filtering flow: ", name)
    with pytest.raises(TypeError, match=name):
        args.mask_array_arg(np.ones((4, 6), np.int32), (4, 6), "Error filtering flow: ", name)
    with pytest.raises(TypeError, match=name):
        args.mask_array_arg([[True] * 6] * 4, (4, 6), "Error filtering flow: ", name)


# ---------------------------------------------------------------------------------------------- the host forms
def test_host_entry_points_check_arguments_before_the_device():
    """Flow.median and median_flow raise for bad arguments without a device (this suite has none)"""
    f = of.Flow.zero((4, 6), 't')
    with pytest.raises(ValueError, match=r"valid.*\(4, 5\).*\(4, 6\)"):
        f.median(valid=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match="only"):
        f.median(only=np.ones((6, 4), bool))
    with pytest.raises(TypeError, match="float32"):
        f.median(3, valid=np.ones((4, 6), np.float32))
    with pytest.raises(TypeError, match="only"):
        f.median(only=[[True] * 6] * 4)
    for bad in (True, 3.0, "3"):
        with pytest.raises(TypeError):
            f.median(bad)
    for bad in (4, 9, 0):
        with pytest.raises(ValueError):
            f.median(bad)
    with pytest.raises(ValueError):
        f.median(3, min_count=10)
    with pytest.raises(ValueError):
        f.median(min_count=0)
    with pytest.raises(TypeError):
        f.median(min_count=1.0)
    vecs, mask = np.zeros((4, 6, 2), np.float32), np.ones((4, 6), bool)
    with pytest.raises(ValueError):
        of.median_flow(vecs, mask, valid=np.ones((6, 4), bool))
    with pytest.raises(TypeError):
        of.median_flow(vecs, mask, only=np.ones((4, 6), np.float64))
    with pytest.raises(ValueError):
        of.median_flow(vecs, mask, ksize=6)
    with pytest.raises(ValueError):
        of.median_flow(vecs, mask, ksize=7, min_count=50)
    assert 'median_flow' in of.flow_operations.__all__ and of.median_flow is of.flow_operations.median_flow


def test_without_a_device_the_host_forms_raise_after_validation():
    if nat.device_count() > 0:
        pytest.skip("a GPU is present")
    f = of.Flow.zero((4, 6), 't')
    with pytest.raises(nat.NoDeviceError):
        f.median()
    with pytest.raises(nat.NoDeviceError):
        f.median(3, valid=np.ones((4, 6), bool), only=np.ones((4, 6), np.uint8), min_count=9)
    with pytest.raises(nat.NoDeviceError):
        of.median_flow(np.zeros((4, 6, 2), np.float32), np.ones((4, 6), bool))
    with pytest.raises(ValueError):                                        # validation comes first
        f.median(4)
    lib = nat.load()
    assert lib.ofl_median_dev(None, None, None, None, 4, 6, 1, 3, 1, None, None, None) == nat.E_NODEVICE
    assert lib.ofl_median(None, None, None, None, 4, 6, 1, 3, 1, None, None) == nat.E_NODEVICE
