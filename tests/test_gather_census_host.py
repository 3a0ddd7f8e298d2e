"""The case table of the image-gather path tests (tests/gather_cases.py) reaches every branch of K1 that it names: proven
here on the CPU by the wave census (tests/gather_census.py), which restates the kernel's own wave-uniform predicates.
tests/test_gpu_gather_paths.py then compares the kernels with the oracle on the same cases.

REQUIRED is the claim: for each class (tokens joined by `+`: one wave must carry all of them) the (type, channels) groups in
which at least one wave of at least one case must fall into it.  UNREACHABLE lists what no input can reach, with the line
of the kernel that says so."""
from collections import defaultdict

import numpy as np
import pytest

import gather_cases as G
import gather_census as gc
from gather_census import U8, I16, U16, F32, F64

EVERY = (1, 2, 3, 4)
ALL = {U8: EVERY, I16: EVERY, U16: EVERY, F32: EVERY, F64: EVERY}
PADDED = {U8: (3,), I16: (3,), U16: (3,)}                                  # 6- and 12-byte runs
JOINABLE = {U8: (1, 3)}                                                    # 2- and 6-byte pixel pairs
XPOSE = {F32: (3, 4)}                                                      # the transposed form
BANDS = {U8: (1, 3), I16: (3,), U16: (2,), F32: (1, 3), F64: (2,)}         # the row-band group

REQUIRED = [
    # --- the flow load
    ('flow:whole', ALL),
    ('flow:whole+offset', ALL),                  # the common wave with padding offsets at the C ABI
    ('flow:whole+offset+fmask', ALL),            # ... and its flow-mask words
    ('flow:aligned', ALL),
    ('flow:aligned+fmask', ALL),
    ('flow:single', ALL),                        # odd pad_left / odd fW: unaligned single loads of the flow
    ('flow:single+flow:straddle', ALL),          # a pixel pair cut by the flow area's edge
    ('flow:single+fmask', ALL),                  # ... and of its mask
    ('flow:none', ALL),
    # --- the three paths
    ('outside', ALL),
    ('border', ALL),
    ('border+smask', ALL),
    ('border+nosmask', ALL),
    ('inside', ALL),
    ('inside+flow:whole', ALL),
    ('inside+smask', ALL),
    ('inside+nosmask', ALL),
    ('inside+px+group4', {U8: EVERY, I16: EVERY, U16: EVERY, F32: (1, 2)}),
    ('inside+px1', {F64: EVERY}),                # float64 in the all-inside wave: gather_px<INSIDE = true>
    ('h1+border', ALL),                          # H < 2 forces inside = false
    ('h1+outside', ALL),
    # --- float32 with 3 / 4 channels: two pixels in flight, un-rotated and transposed
    ('norot+inside+px+group2', XPOSE),
    ('norot+border', XPOSE),
    ('norot+outside', XPOSE),
    ('rot+inside+px+group2', XPOSE),
    ('rot+border', XPOSE),
    ('rot+outside', XPOSE),
    ('rot+flow:whole', XPOSE),
    ('rot+flow:aligned', XPOSE),
    ('rot+flow:single', XPOSE),
    ('rot+val:joined', XPOSE),
    ('rot+val:pair', XPOSE),
    # --- the read-ahead fallback: an all-inside wave one of whose runs ends at the image's end
    ('inside+wide', PADDED),
    ('inside+narrow', PADDED),
    ('inside+narrow+smask', PADDED),
    ('inside+narrow+val:joined', PADDED),
    ('inside+narrow+val:pair', PADDED),
    ('inside+narrow+img:joined', {U8: (3,)}),
    ('inside+narrow+img:pair', {U8: (3,)}),
    ('inside+narrow+sep', {U8: (3,)}),
    ('inside+narrow+fix4', {U8: (3,)}),
    ('inside+narrow+flt', {U8: (3,)}),
    # --- uint8 arithmetic of the all-inside wave
    ('inside+sep', {U8: EVERY}),
    ('inside+fix4', {U8: EVERY}),
    ('inside+flt', {U8: EVERY}),
    # --- the stores: joined dwords (W % 4 == 0) and per pair, met by every path and every flow load
    ('img:joined+inside', JOINABLE), ('img:joined+border', JOINABLE), ('img:joined+outside', JOINABLE),
    ('img:pair+inside', JOINABLE), ('img:pair+border', JOINABLE), ('img:pair+outside', JOINABLE),
    ('img:joined+flow:whole', JOINABLE), ('img:joined+flow:aligned', JOINABLE), ('img:joined+flow:single', JOINABLE),
    ('img:pair+flow:whole', JOINABLE), ('img:pair+flow:aligned', JOINABLE), ('img:pair+flow:single', JOINABLE),
    ('img:joined+h1', JOINABLE), ('img:pair+h1', JOINABLE),
    ('img:own+inside', {U8: (2, 4), I16: EVERY, U16: EVERY, F32: EVERY, F64: EVERY}),
    ('val:joined+inside', ALL), ('val:joined+border', ALL), ('val:joined+outside', ALL),
    ('val:pair+inside', ALL), ('val:pair+border', ALL), ('val:pair+outside', ALL),
    ('val:joined+flow:whole', ALL), ('val:joined+flow:aligned', ALL), ('val:joined+flow:single', ALL),
    ('val:pair+flow:whole', ALL), ('val:pair+flow:aligned', ALL), ('val:pair+flow:single', ALL),
    ('val:joined+fmask', ALL), ('val:pair+fmask', ALL),
    # --- row bands whose first row and height are no multiples of 8: (5, 11), and (16, 3)
    ('band+inside', BANDS), ('band+border', BANDS),
    ('band:odd+inside', BANDS), ('band:odd+border', BANDS),
    ('band+val:joined', BANDS), ('band+val:pair', BANDS),
    ('band:odd+val:joined', BANDS), ('band:odd+val:pair', BANDS),
    ('band:odd+img:joined', JOINABLE), ('band:odd+img:pair', JOINABLE),
]

# (type, arithmetic mode of gather_cases.MODES) -> classes: every (quant, arith, rule) a type is walked with meets the common wave
# with padding offsets, all three paths, and both forms of the validity store
REQUIRED_MODES = ['flow:whole+offset', 'inside', 'border', 'outside', 'val:joined', 'val:pair']

# the folded instantiations gather2_kernel<T, CT, SPEC> are kernels of their own per channel count: (type, mode, C) -> classes
FOLDED = [(U8, 'fix_ge.fold'), (U8, 'rne_gt.fold'), (F32, 'eq.fold')]
REQUIRED_FOLDED = ['inside', 'border', 'outside', 'flow:whole', 'val:joined', 'val:pair']

# routes of launch_gather_t: (route, {type: channels})
REQUIRED_ROUTES = [
    ('paired', ALL),
    ('general_ct', ALL),                         # odd width, 1 - 4 channels: gather_kernel<T, CT>
    ('general_loop', {U8: (6,), I16: (6,), U16: (6,), F32: (6,), F64: (6,)}),      # the runtime channel loop, odd and even width
]

UNREACHABLE = [
    ('flow:aligned+flow:straddle', "pad_left, fW and a lane's first x are even: `inf[2g]` and `inf[2g + 1]` are both set or both clear"),
    ('inside+h1', "gather2_core: `if (H < 2) inside = false;`"),
    ('narrow outside the padded run types', "gather2_core: `wide` is only ever cleared under `if constexpr (kPadded)`"),
    ('rot outside float32 with 3 / 4 channels', "gather2_kernel: `constexpr bool kXp = sizeof(T) == 4 && CT >= 3;`"),
    ('inside+px for float64', "gather2_core: `else if (all_inside && sizeof(T) < 8)`: float64 keeps gather_px<T, CT, true>"),
    ('sep with QUANT_EXACT or FLOAT_RNE', "px_blend: `if (fixed_u8 && sep)`, sep = (quant == OFL_QUANT_OPENCV)"),
    ('any wave class of the general kernel', "gather_kernel has no wave-uniform branch: one pixel per thread, every tap predicated"),
]


@pytest.fixture(scope="module")
def reach():
    """(type, C) -> set of frozensets of tokens; (type, mode) -> the same; (type, C) -> routes; case id -> tokens"""
    by_tc, by_mode, routes, by_case = defaultdict(set), defaultdict(set), defaultdict(set), {}
    by_mode_c = defaultdict(set)
    for c in G.CASES:
        a = G.build(c)
        seen = set()
        for b in range(c['batch']):
            r, tokens, combos = G.census_of(c, a, b)
            routes[(c['dtype'], c['C'])].add(r)
            by_tc[(c['dtype'], c['C'])].update(combos)
            by_mode[(c['dtype'], c['mode'])].update(combos)
            by_mode_c[(c['dtype'], c['mode'], c['C'])].update(combos)
            seen.update(tokens)
        by_case[c['id']] = seen
    return by_tc, by_mode, routes, by_case, by_mode_c


def _has(combos, cls):
    need = frozenset(cls.split('+'))
    return any(need <= k for k in combos)


def test_every_required_class_is_reached(reach):
    by_tc, _, routes, _, _ = reach
    missing = [(dtype, C, cls) for cls, groups in REQUIRED for dtype, chans in groups.items() for C in chans
               if not _has(by_tc[(dtype, C)], cls)]
    missing += [(dtype, C, r) for r, groups in REQUIRED_ROUTES for dtype, chans in groups.items() for C in chans
                if r not in routes[(dtype, C)]]
    assert not missing, missing


def test_every_arithmetic_mode_meets_the_common_wave_and_all_paths(reach):
    _, by_mode, _, _, by_mode_c = reach
    missing = [(dtype, m[0], cls) for dtype, modes in G.MODES.items() for m in modes for cls in REQUIRED_MODES
               if not _has(by_mode[(dtype, m[0])], cls)]
    missing += [(dtype, mode, C, cls) for dtype, mode in FOLDED for C in EVERY for cls in REQUIRED_FOLDED
                if not _has(by_mode_c[(dtype, mode, C)], cls)]
    assert not missing, missing


def test_named_cases_reach_what_their_names_say(reach):
    """the flow kinds do what gather_cases.py builds them for"""
    _, _, _, by_case, _ = reach
    for c in G.CASES:
        t = by_case[c['id']]
        if gc.route(c['dtype'], c['C'], c['H'], c['W'], c['fH'], c['fW']) != 'paired' or c['entry'] != 'single':
            continue
        if c['kind'] == 'corner':
            assert 'inside' in t, c['id']
            if c['dtype'] in (U8, I16, U16) and c['C'] == 3:
                assert 'narrow' in t and ('wide' in t or c['H'] == 2), c['id']      # (2 x 128 is one wave)
        if c['kind'] == 'shift' and c['H'] >= 2:
            assert 'inside' in t and 'rot' not in t, c['id']
        if c['kind'] == 'outside':
            assert 'outside' in t and 'inside' not in t, c['id']
        if c['kind'] == 'shear' and c['dtype'] == F32 and c['C'] >= 3:
            assert 'rot' in t, c['id']
        if c['H'] < 2:
            assert 'h1' in t and 'inside' not in t, c['id']
        if c['place'] == 'odd':
            assert 'flow:single' in t and 'flow:whole' not in t, c['id']


def test_case_limits():
    """small cases (the oracle is instant), unique names"""
    ids = [c['id'] for c in G.CASES]
    assert len(set(ids)) == len(ids)
    for c in G.CASES:
        assert c['H'] <= 40 and c['W'] <= 392, c['id']
        assert 0 <= c['row0'] and c['row0'] + c['rows'] <= c['H'], c['id']
        assert c['pad_top'] + c['fH'] <= c['H'] and c['pad_left'] + c['fW'] <= c['W'], c['id']


def test_oracle_runs_every_case(oracle):
    """a malformed case fails here, not on the GPU; where the census says that no tap is inside, the oracle's image is zero"""
    for c in G.CASES:
        a = G.build(c)
        B, nsrc = c['batch'], 1 if c['shared'] else c['batch']
        assert a['src'].shape == (nsrc, c['H'], c['W'], c['C']) and a['src'].dtype == np.dtype(c['dtype']), c['id']
        assert a['flow'].shape == (B, c['fH'], c['fW'], 2) and a['flow'].dtype == np.float32, c['id']
        assert np.isfinite(a['flow']).all(), c['id']
        img, val = G.expected(c, a, oracle)
        assert img.shape == (B, c['rows'], c['W'], c['C']) and img.dtype == a['src'].dtype, c['id']
        assert (val is None) == (not c['valid']), c['id']
        if val is not None:
            assert val.shape == (B, c['rows'], c['W']) and val.dtype == np.uint8 and val.max() <= 1, c['id']
        if c['kind'] == 'outside' and c['place'] == 'frame':
            assert not img.any() and (val is None or not val.any()), c['id']


def test_census_on_inputs_worked_out_by_hand():
    """16 x 256 uint8 RGB, zero flow: 16 waves, all `whole`.  A pixel's taps are (x, y) and (x + 1, y + 1), so the column x = 255 and
    the row y = 15 are not inside: the 8 waves of the tiles at x = 128 and the wave of rows 14 / 15 at x = 0 are border waves, the
    other 7 inside and wide.  The same frame with every vector at 3e4: 16 waves outside.  Odd width: the general kernel."""
    zero = np.zeros((16, 256, 2), np.float32)
    r, t, combos = gc.census(U8, 3, 16, 256, zero, valid=True)
    assert r == 'paired' and sum(combos.values()) == 16
    assert (t['flow:whole'], t['inside'], t['border'], t['outside'], t['wide'], t['narrow']) == (16, 7, 9, 0, 7, 0)
    assert t['img:joined'] == t['val:joined'] == 16 and t['sep'] == 7 and not t['offset'] and not t['band']
    r, t, _ = gc.census(U8, 3, 16, 256, zero + np.float32(3e4))
    assert (t['outside'], t['inside'], t['border']) == (16, 0, 0)
    # every vector (1, 1), sign -1: taps (x - 1, y - 1) and (x, y).  Column 0 and row 0 hang over the edge -- the 8 waves at x = 0 and
    # the wave of rows 0 / 1 at x = 128 are border waves -- and the wave of rows 14 / 15 at x = 128 ends its last run on the image's
    # last byte: ((15 * 256 + 254) * 3 + 8 > 16 * 256 * 3), so it may not read ahead
    r, t, _ = gc.census(U8, 3, 16, 256, zero + np.float32(1.0), sign=-1)
    assert (t['inside'], t['border'], t['outside'], t['narrow'], t['wide']) == (7, 9, 0, 1, 6)
    assert gc.census(U8, 3, 16, 255, np.zeros((16, 255, 2), np.float32))[0] == 'general_ct'
    assert gc.census(F32, 6, 16, 256, zero)[0] == 'general_loop'
