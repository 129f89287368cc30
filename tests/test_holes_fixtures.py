"""The premises of the hole-filling fixtures (tests/holes_fixtures.py), on the CPU: the loops they give, the sizes of their
patches, that the filled meshes are closed, that the degenerate loops stay finite, that the fixtures tell the offset search
of csrc/mesh_fill.hip from one that takes the first of equal offsets, and that the position bound of tests/test_gpu_holes.py
leaves room for float64 sums in another order and for nothing more."""
import functools

import numpy as np
import pytest

import holes_fixtures as HF
import holes_oracle as HO

CAPS = [None, 20, 9, 3, 2]


@functools.lru_cache(maxsize=None)
def s13(cap):
    vs, faces = HF.fans(HF.S13)
    return vs, faces, HO.fill_holes(vs, faces, cap)


@functools.lru_cache(maxsize=None)
def single(n, shift=0.0):
    vs, faces = HF.fans([n], shift=shift)
    return vs, faces, HO.fill_holes(vs, faces)


def sizes_of(faces):
    return [len(l) for l in HO.boundary_loops(faces)]


def test_loop_sizes_come_out_in_list_order():
    for sizes in (HF.S13, [40, 3, 9, 40], [3], [3 + i % 21 for i in range(300)]):
        vs, faces = HF.fans(sizes)
        assert sizes_of(faces) == list(sizes)
        assert vs.dtype == np.float32 and faces.dtype == np.int64 and vs.shape[0] == sum(n if n == 3 else n + 1 for n in sizes)
        assert int(faces.max()) == vs.shape[0] - 1 and HO.half_edge_stats(faces)[0] == 1


def test_ring_count_changes_where_s13_has_a_loop_on_both_sides():
    for lo, hi in ((9, 10), (15, 16), (21, 22)):
        assert HO.ring_count(hi) == HO.ring_count(lo) + 1 and lo in HF.S13 and hi in HF.S13
    assert [HO.ring_count(n) for n in (4, 9, 10, 15, 16, 21, 22, 40)] == [1, 1, 2, 2, 3, 3, 4, 6]


def test_a_permutation_reorders_and_interleaves_the_loops():
    vs, faces = HF.fans(HF.S13)
    p_vs, p_faces = HF.fans(HF.S13, perm=5)
    loops = HO.boundary_loops(p_faces)
    assert sorted(len(l) for l in loops) == sorted(HF.S13) and [len(l) for l in loops] != HF.S13
    assert np.array_equal(np.sort(p_vs.view(np.uint32), 0), np.sort(vs.view(np.uint32), 0))       # the same points
    # in the sorted boundary array a loop's vertices are its ids: the ranges of two loops overlap
    spans = [(min(l), max(l)) for l in loops]
    assert sum(a[0] < b[0] < a[1] for a in spans for b in spans) >= len(loops)
    big = [l for l in loops if len(l) == 40]
    assert len(big) == 2 and min(big[1]) < max(big[0])


@pytest.mark.parametrize("cap", CAPS)
def test_s13_counts_and_what_stays_open(cap):
    vs, faces, (w_vs, w_faces, inserted, filled, loops) = s13(cap)
    assert (w_vs.shape[0] - vs.shape[0], w_faces.shape[0] - faces.shape[0]) == HF.S13_COUNTS[cap]
    assert filled.tolist() == [cap is None or n <= cap for n in HF.S13]
    assert sizes_of(w_faces) == [n for n in HF.S13 if cap is not None and n > cap]
    assert HO.half_edge_stats(w_faces)[0] == 1
    if cap is None:
        assert HO.half_edge_stats(w_faces) == (1, 0)


@pytest.mark.parametrize("n", list(HF.SINGLE_COUNTS))
def test_single_loop_counts_and_closedness(n):
    vs, faces, (w_vs, w_faces, _, filled, loops) = single(n)
    assert [len(l) for l in loops] == [n] and filled.tolist() == [True]
    assert (w_vs.shape[0] - vs.shape[0], w_faces.shape[0] - faces.shape[0]) == HF.SINGLE_COUNTS[n]
    assert HO.half_edge_stats(w_faces) == (1, 0)


def test_coincident_premises():
    vs, faces, loops = HF.coincident()
    a, b, c = loops
    seg = np.linalg.norm(np.roll(vs[a], -1, 0).astype(np.float64) - vs[a], axis=1)
    assert np.flatnonzero(seg == 0).tolist() == [0, 9, 10, 23]          # first, two in a row, closing
    assert (vs[b] == vs[b[0]]).all() and float(np.abs(vs[c]).min()) > 9e3 and float(np.abs(vs[a + b]).max()) < 10
    w_vs, w_faces, _, filled, w_loops = HO.fill_holes(vs, faces)
    assert w_loops == loops and filled.all() and np.isfinite(w_vs).all()
    assert HO.half_edge_stats(w_faces) == (1, 0)
    V = vs.shape[0]
    first = V + sum(HO.ring_sizes(24)[1:])
    count = sum(HO.ring_sizes(12)[1:])
    point = vs[b[0]].astype(np.float64)
    assert count == 7 and np.array_equal(w_vs[first:first + count], np.repeat(point[None], count, 0))


# ---- sensitivity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_table_form_equals_the_oracle(cap):
    vs, faces, (w_vs, w_faces, _, _, loops) = s13(cap)
    got_faces, got_places = HF.table_form(vs.shape[0], loops, cap)
    assert np.array_equal(got_faces, w_faces[faces.shape[0]:])
    assert np.array_equal(got_places, HF.expected_places(loops, cap)) and got_places.shape[0] == w_vs.shape[0] - vs.shape[0]


@pytest.mark.parametrize("cap", [20, 9, 3])
def test_first_of_equal_offsets_is_told_apart(cap):
    vs, faces, (w_vs, w_faces, _, _, loops) = s13(cap)
    try:
        got_faces, _ = HF.table_form(vs.shape[0], loops, cap, ties="first")
    except (IndexError, ZeroDivisionError):
        return                                                   # a read outside a table
    assert not np.array_equal(got_faces, w_faces[faces.shape[0]:])


def test_first_of_equal_offsets_is_told_apart_on_the_other_fixtures():
    """fans([40, 3, 9, 40]) at cap 20 (open loops first and last) shows it in the faces; the permuted S13 too.  Uncapped S13
    has no equal face offsets (a triangle adds a face) but equal vertex offsets: the places of the new vertices show it."""
    for sizes, perm, cap in (([40, 3, 9, 40], None, 20), (HF.S13, 5, 20)):
        vs, faces = HF.fans(sizes, perm=perm)
        w_vs, w_faces, _, _, loops = HO.fill_holes(vs, faces, cap)
        assert np.array_equal(HF.table_form(vs.shape[0], loops, cap)[0], w_faces[faces.shape[0]:])
        try:
            assert not np.array_equal(HF.table_form(vs.shape[0], loops, cap, ties="first")[0], w_faces[faces.shape[0]:])
        except (IndexError, ZeroDivisionError):
            pass
    vs, faces, (_, _, _, _, loops) = s13(None)
    try:
        assert not np.array_equal(HF.table_form(vs.shape[0], loops, None, ties="first")[1], HF.expected_places(loops, None))
    except (IndexError, ZeroDivisionError):
        pass


# ---- the position bound ----------------------------------------------------------------------------------------------------
def position_cases():
    yield "513", single(513)[0], single(513)[2]
    yield "1025", single(1025)[0], single(1025)[2]
    yield "257 + 1e4", single(257, 1e4)[0], single(257, 1e4)[2]
    vs, faces, _ = HF.coincident()
    yield "coincident", vs, HO.fill_holes(vs, faces)


def test_position_bound_holds_for_another_float64_order():
    """2^-23 max|coordinate|: half of it is the one rounding to float32, the other half is there for the order of the float64
    sums, which needs 2^-29 of it.  A float32 intermediate would not fit: see the last assertion."""
    for name, vs, (w_vs, _, _, _, loops) in position_cases():
        V = vs.shape[0]
        got = HF.positions_other_order(vs, loops)
        assert got.dtype == np.float32 and got.shape == w_vs[V:].shape
        err = float(np.abs(got.astype(np.float64) - w_vs[V:]).max())
        bound = 2.0 ** -23 * float(np.abs(vs).max())
        print(f"{name}: max|err| {err:.3e} = {err / bound:.2f} of the bound {bound:.3e}")
        assert err <= bound
        assert err > 0.125 * bound                                   # the bound is not slack: the rounding alone takes a quarter
    # the same positions from float32 arc lengths miss the bound
    vs, _, (w_vs, _, _, _, loops) = single(1025)
    b = vs[loops[0]].astype(np.float64)
    seg32 = np.linalg.norm(np.roll(b, -1, 0) - b, axis=1).astype(np.float32)
    cum32 = np.concatenate([[0], np.cumsum(seg32, dtype=np.float32)]).astype(np.float64)
    n, sizes = 1025, HO.ring_sizes(1025)
    s = np.arange(sizes[1]) / sizes[1] * cum32[-1]
    i = np.minimum(np.searchsorted(cum32, s, side="right") - 1, n - 1)
    t = ((s - cum32[i]) / seg32[i])[:, None]
    p = b[i] * (1 - t) + b[(i + 1) % n] * t
    ring1 = (p + (1 / (len(sizes) - 1)) * (b.mean(0) - p)).astype(np.float32)
    err = float(np.abs(ring1.astype(np.float64) - w_vs[vs.shape[0]:vs.shape[0] + sizes[1]]).max())
    assert err > 2.0 ** -23 * float(np.abs(vs).max())
