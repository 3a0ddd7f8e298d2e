"""tests/view_cases.py on a CPU: the placements have the residues they claim, the shapes cross the sizes at which the
kernels change their work split, and the poison is not vacuous -- a kernel that took one pixel from outside its view
would give another statistics word, another visualise range and other K8 moments, on every shape."""
import os
import re

import numpy as np
import pytest

import matrix_ref
import stream_ref
import view_cases as V
import visualise_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oflibnumpy_amd", "csrc")


def source_number(name, pattern):
    with open(os.path.join(CSRC, name)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, (name, pattern, found)
    return int(found[0])


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_placements_have_their_residues_and_their_poison(shape):
    v, m = V.random_case(shape)
    n = shape[0] * shape[1]
    ps = V.placements(v, m)
    assert [(p.rv, p.rm) for p in ps] == V.RESIDUES and len(set(V.RESIDUES)) == 8
    for p in ps:
        assert (p.voff % 16, p.moff % 4) == (p.rv, p.rm)
        assert p.vimg.dtype == np.uint8 and p.mimg.dtype == np.uint8 and p.vimg.size % 16 == 0 and p.mimg.size % 16 == 0
        assert p.voff >= V.GUARD and p.vimg.size - (p.voff + 8 * n) >= V.GUARD
        assert p.moff >= V.GUARD and p.mimg.size - (p.moff + n) >= V.GUARD
        got_v, got_m = V.window(p)
        assert got_v.tobytes() == v.tobytes() and got_m.tobytes() == m.tobytes()
        for poison in (p.vimg[:p.voff].view(np.uint32), p.vimg[p.voff + 8 * n:].view(np.uint32)):
            assert np.all(poison[0::2] == V.QNAN_BITS) and np.all(poison[1::2].view(np.float32) == V.BIG)
        front, back = p.mimg[:p.moff], p.mimg[p.moff + n:]
        for poison in (front, back):
            assert set(np.unique(poison)) == {0x00, 0xFF} and np.all(poison[1:] != poison[:-1])
        first, last = m.reshape(-1)[0], m.reshape(-1)[-1]
        assert bool(front[-1]) != bool(first) and front[-1] != first
        assert bool(back[0]) != bool(last) and back[0] != last


def test_shapes_cross_the_sizes_where_the_work_split_changes():
    fit_chunk = source_number("ofl_fit.hip", r"// (\d+) px per chunk")
    select_block = source_number("ofl_visualise.hip", r"// (\d+) px per workgroup")
    stats_wg = source_number("ofl_stats.hip", r"constexpr int kStatChunks = (\d+);") * 256 * 2    # pairs per thread, 256 threads
    assert (fit_chunk, select_block, stats_wg) == (4096, 8192, 4096)
    px = [h * w for h, w in V.SHAPES]
    assert px == [1961, 8241, 35, 3, 1]
    assert px[1] > max(fit_chunk, select_block, stats_wg) and px[1] % 2 == 1
    assert px[0] < min(fit_chunk, select_block, stats_wg)
    assert (px[0] % 4, px[2] % 4) == (1, 3) and px[0] % 2 == 1
    assert V.SHAPES[0] == (37, 53)                                  # the batch shape of test_gpu_stream.batch_of_three
    # field 1 of a batch of an odd shape: vectors 8 off, mask at an odd address; (5, 7): 35 % 4 == 3
    assert [(px[i] * 8 % 16, px[i] % 4) for i in (0, 2)] == [(8, 1), (8, 3)] == V.ODD_RESIDUES


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_one_poison_pixel_changes_every_answer(shape):
    v, m = V.random_case(shape)
    for p in V.placements(v, m, V.ODD_RESIDUES):
        fv, fm = V.window(p)
        word = stream_ref.stats_word(fv, fm)
        f = visualise_ref.thresholded(fv)
        rng = visualise_ref.default_range(visualise_ref.magnitude(f[..., 0], f[..., 1]))
        assert np.isfinite(rng) and not word & stream_ref.NONFINITE
        for shift in (-1, 1):
            sv, sm = V.window(p, shift)
            assert stream_ref.stats_word(sv, sm) != word, (shape, shift)
            with np.errstate(all='ignore'):
                f = visualise_ref.thresholded(sv)
                assert visualise_ref.default_range(visualise_ref.magnitude(f[..., 0], f[..., 1])) != rng, (shape, shift)
    for kind, ref in (('holes', 's'), ('noisy', 't')):
        v, m = V.matrix_case(kind, shape, ref)
        for p in V.placements(v, m, V.ODD_RESIDUES):
            fv, fm = V.window(p)
            want = matrix_ref.Field(fv, ref, fm).moments()
            assert np.array_equal(want, matrix_ref.Field(v, ref, m).moments())
            for shift in (-1, 1):
                sv, sm = V.window(p, shift)
                with np.errstate(all='ignore'):
                    assert not np.array_equal(matrix_ref.Field(sv, ref, sm).moments(), want), (kind, shape, shift)
