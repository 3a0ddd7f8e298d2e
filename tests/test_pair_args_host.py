"""The argument surface the image-pair families K21 ... K24 and K26 share, without a GPU: the messages of the host path of
Flow.photometric / census / ssim / refine / inverse_search that are raised before any native call, and those of the number
checks of the args.*_args functions of K21 ... K24 (K26's: test_ssim_host.py).  Every expected string is written out."""
import re

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd.args import photometric_args, census_args, refine_args, inverse_search_args

F32 = np.float32
H, W = 6, 9

PREFIX = {'photometric': "Error computing photometric error: ", 'census': "Error computing census distance: ",
          'ssim': "Error computing structural similarity: ", 'refine': "Error refining flow: ",
          'inverse_search': "Error searching flow: "}
METHODS = sorted(PREFIX)


def _call(method, near, far, **kw):
    return getattr(of.Flow.zero((H, W), 't'), method)(near, far, **kw)


def _raises(kind, text):
    return pytest.raises(kind, match="^" + re.escape(text) + "$")


def _img(*shape, dtype=F32):
    return np.zeros(shape, dtype)


@pytest.mark.parametrize("method", METHODS)
def test_shared_host_path_messages(method):
    p = PREFIX[method]
    with _raises(ValueError, p + "the arrays need the same shape, got (6, 9, 3) and (6, 9, 2)"):
        _call(method, _img(H, W, 3), _img(H, W, 2))
    with _raises(TypeError, p + "the arrays need the same dtype, got float32 and float16"):
        _call(method, _img(H, W, 3), _img(H, W, 3, dtype=np.float16))
    with _raises(TypeError, p + "near needs to have dtype float32, float16 or uint8, got float64"):
        _call(method, _img(H, W, 3, dtype=np.float64), _img(H, W, 3))
    with _raises(TypeError, p + "far needs to have dtype float32, float16 or uint8, got float64"):
        _call(method, _img(H, W, 3), _img(H, W, 3, dtype=np.float64))
    with _raises(ValueError, p + "layout must be 'chw' or 'hwc', got 'xyz'"):
        _call(method, _img(H, W, 3), _img(H, W, 3), layout='xyz')
    with _raises(ValueError, p + "arrays and flow need the same height and width, got (6, 8) and (6, 9)"):
        _call(method, _img(H, 8, 3), _img(H, 8, 3))
    with _raises(ValueError, p + "arrays and flow need the same height and width, got (9, 6) and (6, 9)"):
        _call(method, _img(3, W, H), _img(3, W, H), layout='chw')


@pytest.mark.parametrize("method", ['census', 'ssim', 'refine', 'inverse_search'])
def test_channel_limit_message(method):
    with _raises(ValueError, PREFIX[method] + "the tensors need 1 to 4 channels (grey, two-plane, RGB, RGBA), got 5"):
        _call(method, _img(H, W, 5), _img(H, W, 5))
    with _raises(ValueError, PREFIX[method] + "the tensors need 1 to 4 channels (grey, two-plane, RGB, RGBA), got 5"):
        _call(method, _img(5, H, 8), _img(5, H, 8), layout='chw')             # before the height / width check


@pytest.mark.parametrize("method", ['refine', 'inverse_search'])
def test_one_item_message(method):
    with _raises(ValueError, PREFIX[method] + "one flow takes one item, got 2"):
        _call(method, _img(2, H, W, 3), _img(2, H, W, 3))
    with _raises(ValueError, PREFIX[method] + "one flow takes one item, got 2"):
        _call(method, _img(2, H, 8, 3), _img(2, H, 8, 3))                     # before the height / width check


@pytest.mark.parametrize("method", ['photometric', 'census', 'ssim', 'refine'])
def test_mask_messages(method):
    p = PREFIX[method]
    with _raises(ValueError, p + "near_mask needs to have the shape of the flow, got (9, 6) and (6, 9)"):
        _call(method, _img(H, W, 3), _img(H, W, 3), near_mask=np.ones((W, H), np.bool_))
    with _raises(ValueError, p + "far_mask needs to have the shape of the flow, got (6, 8) and (6, 9)"):
        _call(method, _img(H, W, 3), _img(H, W, 3), far_mask=np.ones((H, 8), np.uint8))
    with _raises(TypeError, p + "near_mask needs to have dtype bool or uint8, got float32"):
        _call(method, _img(H, W, 3), _img(H, W, 3), near_mask=np.ones((H, W), F32))


# ---------------------------------------------------------------------------------------------- the number checks
def test_photometric_args_numbers():
    p = PREFIX['photometric']
    with _raises(TypeError, p + "eps must be a number or None, got bool"):
        photometric_args(eps=True)
    with _raises(TypeError, p + "threshold must be a number or None, got str"):
        photometric_args(threshold="1")
    with _raises(ValueError, p + "eps must be finite and not negative, got nan"):
        photometric_args(eps=float('nan'))
    with _raises(ValueError, p + "threshold must be finite and not negative, got -1"):
        photometric_args(threshold=-1)
    with _raises(ValueError, p + "eps must be finite and not negative, got 1e+39"):
        photometric_args(eps=1e39)
    code, eps, thr = photometric_args('l2', 0, 2)
    assert (eps, thr) == (F32(0), F32(2)) and type(eps) is np.float32 and type(thr) is np.float32
    assert photometric_args()[1:] == (F32(1e-3), None)


def test_census_args_numbers():
    p = PREFIX['census']
    with _raises(TypeError, p + "noise must be a number or None, got bool"):
        census_args(noise=True)
    with _raises(ValueError, p + "knee must be finite and positive, got nan"):
        census_args(knee=float('nan'))
    with _raises(ValueError, p + "noise must be finite and positive, got -1"):
        census_args(noise=-1)
    with _raises(ValueError, p + "noise must be finite and positive, got 0"):
        census_args(noise=0)
    with _raises(ValueError, p + "noise must be finite and positive, got 1e-50"):
        census_args(noise=1e-50)                                              # 0 once rounded to float32
    with _raises(ValueError, p + "delta must be finite and not negative, got -1"):
        census_args(mode='hard', delta=-1)
    with _raises(ValueError, p + "threshold must be finite and not negative, got 1e+39"):
        census_args(threshold=1e39)
    with _raises(TypeError, p + "window must be an integer, got bool"):
        census_args(window=True)
    with _raises(TypeError, p + "min_count must be an integer or None, got float"):
        census_args(min_count=2.0)
    with _raises(ValueError, p + "min_count must be in [1, 24] for window 5, got 25"):
        census_args(window=5, min_count=25)
    with _raises(ValueError, p + "min_count must be in [1, 48] for window 7, got 0"):
        census_args(min_count=0)
    assert census_args(mode='hard', delta=0)[2:4] == (F32(0), F32(0))


def test_refine_args_numbers():
    p = PREFIX['refine']
    with _raises(TypeError, p + "alpha must be a number or None, got bool"):
        refine_args(alpha=True)
    with _raises(ValueError, p + "alpha must be finite and not negative, got nan"):
        refine_args(alpha=float('nan'))
    with _raises(ValueError, p + "delta must be finite and not negative, got -1"):
        refine_args(delta=-1)
    with _raises(ValueError, p + "alpha must be finite and not negative, got 1e+39"):
        refine_args(alpha=1e39)
    with _raises(ValueError, p + "zeta must be finite and positive (its float32 square too), got 1e-30"):
        refine_args(zeta=1e-30)
    with _raises(ValueError, p + "omega must lie in (0, 2), got 2"):
        refine_args(omega=2)
    with _raises(TypeError, p + "sor must be an integer or None, got bool"):
        refine_args(sor=True)
    with _raises(TypeError, p + "fixed_point must be an integer or None, got float"):
        refine_args(fixed_point=1.0)
    with _raises(ValueError, p + "fixed_point must be in [1, 32], got 0"):
        refine_args(fixed_point=0)
    with _raises(ValueError, p + "sor must be in [1, 32], got 33"):
        refine_args(sor=33)
    assert refine_args(alpha=0, delta=0)[:2] == (F32(0), F32(0))


def test_inverse_search_args_numbers():
    p = PREFIX['inverse_search']
    with _raises(TypeError, p + "floor must be a number, got bool"):
        inverse_search_args(floor=True)
    with _raises(TypeError, p + "floor must be a number, got NoneType"):
        inverse_search_args(floor=None)
    with _raises(ValueError, p + "floor must be finite and positive (as float32 too), got nan"):
        inverse_search_args(floor=float('nan'))
    with _raises(ValueError, p + "floor must be finite and positive (as float32 too), got -1"):
        inverse_search_args(floor=-1)
    with _raises(ValueError, p + "floor must be finite and positive (as float32 too), got 1e+39"):
        inverse_search_args(floor=1e39)
    with _raises(ValueError, p + "floor must be finite and positive (as float32 too), got 1e-50"):
        inverse_search_args(floor=1e-50)
    with _raises(TypeError, p + "iterations must be an integer, got bool"):
        inverse_search_args(iterations=True)
    with _raises(TypeError, p + "stride must be an integer, got float"):
        inverse_search_args(stride=4.0)
    with _raises(ValueError, p + "iterations must be in [1, 32], got 33"):
        inverse_search_args(iterations=33)
    with _raises(ValueError, p + "iterations must be in [1, 32], got 0"):
        inverse_search_args(iterations=0)
    assert inverse_search_args(4, 4, 1, False, 2) == (4, 4, 1, False, F32(2))
