"""CPU suite: the cases of tests/nonfinite_cases.py reach what they claim, and the oracle does on them what include/ofl.h
promises of the device -- a vector with a non-finite component samples nothing: every tap outside, the pixel invalid.  The
oracle itself runs over the same cases as a stand-alone program under AddressSanitizer and UBSan with float-cast-overflow."""
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as C
import nonfinite_cases as N
from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTS = [O.QUANT_OPENCV, O.QUANT_EXACT]
SIGNS = [-1, 1]
ALL = [(s, k, p) for s in N.SHAPES for k in N.KINDS for p in N.PLACEMENTS]
IDS = ["{}x{}x{}-{}-{}".format(*s, k, p) for s, k, p in ALL]


def reach(c, quant):
    """{(layout, class, pattern): bad pixels} of a built case, the classes from the clean field under `quant`"""
    n = {}
    for b in range(c['shape'][0]):
        for layout, cls, px in N.waves(c['clean'][b], c['sign'], quant):
            for q in px:
                p = int(c['bad'][b][q])
                if p >= 0:
                    n[(layout, cls, p)] = n.get((layout, cls, p), 0) + 1
    return n


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("quant", QUANTS)
def test_every_pattern_reaches_every_wave_class(sign, quant):
    """Over the tiled shapes (even W) of the 'class' placement: every pattern sits in a streamed wave of every class, and in a
    block wave (rotated tile) of every class the rotated fields have -- mixed, the border path, among them."""
    total, block_classes = {}, set()
    for shape in N.SHAPES:
        if shape[2] % 2:
            continue
        for kind in N.KINDS:
            c = N.case(shape, kind, 'class', sign)
            assert c['reach'] == reach(c, O.QUANT_OPENCV)            # the placement's own count is the recount
            for k, v in reach(c, quant).items():
                total[k] = total.get(k, 0) + v
            block_classes |= {cls for layout, cls, _ in N.waves(c['clean'][0], sign, quant) if layout == 'block'}
    assert 'mixed' in block_classes
    for p, name in enumerate(N.NAMES):
        for cls in N.CLASSES:
            assert total.get(('stream', cls, p), 0) >= 1, (name, cls)
        for cls in block_classes:
            assert total.get(('block', cls, p), 0) >= 1, (name, cls, 'block')


def test_every_case_holds_every_pattern_it_has_room_for():
    for shape, kind, placement in ALL:
        for sign in SIGNS:
            c = N.case(shape, kind, placement, sign)
            n_px = int(np.prod(shape))
            have = set(c['bad'][c['bad'] >= 0].tolist())
            if placement == 'sprinkle' or n_px >= 37 * len(N.PATTERNS):
                assert len(have) == min(len(N.PATTERNS), n_px), (shape, kind, placement)
            assert have, (shape, kind, placement)                   # (a field of a few pixels: as many as its waves take)
            got = c['fb'].view(np.uint32)[c['bad'] >= 0]
            assert np.array_equal(got, N.BITS[c['bad'][c['bad'] >= 0]])       # bit for bit: payloads, the signalling NaN
            assert np.array_equal(c['fb'][c['bad'] < 0], c['clean'][c['bad'] < 0])


def test_wave_classes_are_the_oracles():
    """With every source pixel valid the oracle's mask is its own statement of the classes: set on every pixel of an inside
    wave, clear on every pixel of an outside one."""
    for shape in N.SHAPES:
        for kind in N.KINDS:
            for sign in SIGNS:
                c = N.case(shape, kind, 'class', sign)
                ones = np.ones(shape[1:], np.uint8)
                for quant in QUANTS:
                    _, m = O.compose3_raw(c['fa'][0], ones, c['clean'][0], ones, sign, quant)
                    for _, cls, px in N.waves(c['clean'][0], sign, quant):
                        ys, xs = np.array(px).T
                        if cls == 'inside' and quant == O.QUANT_OPENCV:      # (un-snapped weights need not sum to exactly 1)
                            assert m[ys, xs].all(), (shape, kind, sign, quant)
                        if cls == 'outside':
                            assert not m[ys, xs].any(), (shape, kind, sign, quant)


@pytest.mark.parametrize("shape,kind,placement", ALL, ids=IDS)
def test_oracle_samples_nothing_at_a_bad_vector(shape, kind, placement):
    for sign in SIGNS:
        c = N.case(shape, kind, placement, sign)
        bad = c['bad'] >= 0
        nonfinite = np.isin(c['bad'], N.NONFINITE)
        for quant in QUANTS:
            for b in range(shape[0]):
                fa, ma, fb, mb, clean = (c[k][b] for k in ('fa', 'ma', 'fb', 'mb', 'clean'))
                tag = (shape, kind, placement, sign, quant, b)
                out, m = O.compose3_raw(fa, ma, fb, mb, sign, quant)
                out0, m0 = O.compose3_raw(fa, ma, clean, mb, sign, quant)
                smp, val = O.gather_bilinear(fa, fb, sign, smask=ma, want_valid=True, quant=quant)
                smp0, val0 = O.gather_bilinear(fa, clean, sign, smask=ma, want_valid=True, quant=quant)
                with np.errstate(invalid='ignore', over='ignore'):
                    con, cov, res, cnt = C.consistency(fb, mb, fa, ma, sign, quant=quant)
                    con0, cov0, res0, _ = C.consistency(clean, mb, fa, ma, sign, quant=quant)
                # mask / valid / covered = 0 at every bad pixel
                assert not m[bad[b]].any() and not val[bad[b]].any() and not cov[bad[b]].any() and not con[bad[b]].any(), tag
                assert not res[bad[b]].any() and cnt == (int(cov.sum()), int(con.sum())), tag
                if quant == O.QUANT_OPENCV:
                    # the sampled term is 0: +0.0 from the gather, and the composition returns the vector itself
                    assert not smp[bad[b]].view(np.uint32).any(), tag
                    assert N.same_floats(out[bad[b]], fb[bad[b]]), tag
                else:
                    # un-snapped: a NaN or Inf coordinate has no fraction; its weights and its blend of four zeros are NaN
                    assert np.isnan(smp[nonfinite[b]]).all() and np.isnan(out[nonfinite[b]]).all(), tag
                    far = bad[b] & ~nonfinite[b]
                    assert not smp[far].view(np.uint32).any() and N.same_floats(out[far], fb[far]), tag
                # every other pixel: the clean field's answer (the sampled data is clean, so no tap holds a bad value)
                good = ~bad[b]
                for got, want in ((out, out0), (smp, smp0), (res, res0)):
                    assert np.array_equal(got[good].view(np.uint32), want[good].view(np.uint32)), tag
                for got, want in ((m, m0), (val, val0), (cov, cov0), (con, con0)):
                    assert np.array_equal(got[good], want[good]), tag


def test_exact_clamp_sends_nan_to_the_lowest_tap():
    """QUANT_EXACT: fmax / fmin take NaN to -32768 before the cast, -Inf as well, +Inf to 32767: no tap inside, value 0 * NaN"""
    src = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    for u, v in ((np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf)):
        flow = np.zeros((3, 4, 2), np.float32)
        flow[1, 2] = u, v
        for sign in SIGNS:
            out, valid = O.gather_bilinear(src, flow, sign, want_valid=True, quant=O.QUANT_EXACT)
            assert np.isnan(out[1, 2]) and not valid[1, 2]
            keep = np.ones((3, 4), bool)
            keep[1, 2] = False
            assert np.array_equal(out[keep], src[keep]) and valid[keep].all()


def test_a_tap_of_weight_zero_carries_its_nan():
    """NaN / Inf in the SAMPLED data under finite flows: 0 * NaN and 0 * Inf are NaN, as in cv2.remap's four products"""
    fa, ma, fb, mb = N.poisoned_source()
    src = np.zeros((2, 3, 2), np.float32)
    src[0, 1] = np.nan, np.inf
    out = O.gather_bilinear(src, np.zeros((2, 3, 2), np.float32) + np.float32(1e-3), -1)      # tap (0, 0), weight 0 on (0, 1)
    assert np.isnan(out[0, 0]).all() and not np.isfinite(out[0, 1]).any()
    for quant in QUANTS:
        o, _ = O.compose3_raw(fa[0], ma[0], fb[0], mb[0], -1, quant)
        ix, iy = N.taps(fb[0], -1, quant)
        H, W = ix.shape
        inside = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2)
        hit = np.zeros((H, W), bool)                                 # a non-finite value in one of the four taps
        bad = ~np.isfinite(fa[0]).all(-1)
        ys, xs = np.nonzero(inside)
        for dy in (0, 1):
            for dx in (0, 1):
                hit[ys, xs] |= bad[iy[ys, xs] + dy, ix[ys, xs] + dx]
        assert hit.sum() > 20 and (~np.isfinite(o[hit]).all(-1)).all(), quant


def test_oracle_is_clean_under_the_sanitizers(tmp_path):
    exe, blob = tmp_path / "nonfinite_oracle_cpu", tmp_path / "cases.bin"
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "nonfinite_oracle_cpu.c"), "-lm"])
    records = 0
    with open(blob, "wb") as f:
        fields = [tuple(N.case(s, k, p, sign)[n] for n in ('fa', 'ma', 'fb', 'mb')) for s, k, p in ALL for sign in SIGNS]
        fields.append(N.poisoned_source())
        for fa, ma, fb, mb in fields:
            for b in range(fa.shape[0]):
                f.write(np.array(fa.shape[1:3], np.int32).tobytes())
                for a in (fa[b], fb[b], ma[b], mb[b]):
                    f.write(np.ascontiguousarray(a).tobytes())
                records += 1
    run = subprocess.run([str(exe), str(blob)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("{} records ok".format(records)), run.stdout
