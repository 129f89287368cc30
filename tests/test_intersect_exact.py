"""The numpy restatement of the self-intersection predicate (tests/intersect_oracle.py) against the exact rational
definition of "two faces cross" (tests/exact_intersect.py), and the conditions the inputs of tests/test_gpu_repair.py
have to meet.  No GPU.  The conditions are properties of the INPUTS (fixed seeds), so that a later change of a generator
cannot quietly empty a class the device tests rely on; the class counts come from the exact definition alone."""
import functools

import numpy as np
import pytest

import exact_intersect as EX
import intersect_oracle as IO

SUBSET = 40            # clusters the exact definition is run on where the whole input is not needed


def agree(vs, faces):
    """restatement == exact definition in pairs and n_degenerate; returns the restatement's result."""
    want = IO.self_intersections(vs, faces)
    pairs, n_deg = EX.self_intersections_exact(vs, faces)
    assert np.array_equal(want.pairs, pairs) and want.n_degenerate == n_deg
    return want


@functools.lru_cache(maxsize=None)
def soups():
    vs, faces = IO.soup_clusters(125)
    pairs, n_deg = EX.self_intersections_exact(vs, faces)
    return vs, faces, pairs, n_deg


@functools.lru_cache(maxsize=None)
def orbit():
    return IO.hand_case_orbit()


# ---- the definition against the hand answers and the restatement --------------------------------------------------------------
def test_exact_definition_gives_the_hand_answers_in_every_labelling():
    vs, faces, pairs, n_deg = orbit()
    assert faces.shape[0] == 3 * (9 * 72 * 2 + 36 * 3) and np.abs(vs).max() <= 2 ** 10
    got, got_deg = EX.self_intersections_exact(vs, faces)
    assert np.array_equal(got, pairs) and got_deg == n_deg == 3 * 36 * 2


def test_restatement_gives_the_hand_answers_in_every_labelling():
    vs, faces, pairs, n_deg = orbit()
    want = IO.self_intersections(vs, faces)
    assert np.array_equal(want.pairs, pairs) and want.n_degenerate == n_deg


def test_restatement_equals_exact_on_the_soups():
    vs, faces, pairs, n_deg = soups()
    want = IO.self_intersections(vs, faces)
    assert np.array_equal(want.pairs, pairs) and want.n_degenerate == n_deg
    assert len(EX.candidates(vs, faces)) < 10000


def test_restatement_equals_exact_on_dyadic_floats():
    vs, faces, _, _ = soups()
    fv = IO.dyadic(vs)
    assert fv.dtype == np.float32 and (fv != np.rint(fv)).any()
    agree(fv, faces[:12 * SUBSET])
    assert np.array_equal(IO.self_intersections(fv, faces).pairs, soups()[2])       # a dyadic scale and shift change no verdict


@pytest.mark.parametrize("sign", [1, -1])
def test_restatement_equals_exact_at_the_limit_of_exactness(sign):
    vs, faces, pairs, _ = soups()
    lv = IO.shifted_to_limit(vs, sign)
    assert (lv.max(0) == 1024).all() if sign > 0 else (lv.min(0) == -1024).all()
    agree(lv, faces[:12 * SUBSET])
    want = IO.self_intersections(lv, faces)
    assert np.array_equal(want.pairs, pairs)                      # a translation changes no verdict
    as_float = IO.self_intersections(lv.astype(np.float32), faces)     # the float64 path the device takes: still exact
    assert np.array_equal(as_float.pairs, pairs) and as_float.n_degenerate == want.n_degenerate


def test_restatement_equals_exact_on_the_coincident_stack():
    vs, faces = IO.coincident_stack(70)
    want = agree(vs, faces)
    assert len(want) == 70 * 69 // 2 and want.face_mask.all() and want.n_degenerate == 0
    assert len(np.unique(vs[faces].reshape(70, 9), axis=0)) == 1 and len(np.unique(faces)) == 210


@pytest.mark.parametrize("big_first", [True, False])
def test_restatement_equals_exact_on_the_ladder(big_first):
    vs, faces = IO.ladder(big_first)
    want = agree(vs, faces)
    big = 0 if big_first else faces.shape[0] - 1
    assert len(want) > 0 and (want.pairs == big).any(1).all()      # which rungs the big face meets is the exact oracle's say


# ---- the conditions on the inputs --------------------------------------------------------------------------------------------
def _slot_not_in(f, g):
    return [k for k in range(3) if f[k] not in g]


def test_the_soups_fill_every_class_of_the_predicate():
    """Counted with the exact definition only.  Seed 2024 (the first one tried), n = 125:
    classes (shared ids, pair) (0, no) 232, (0, yes) 406, (1, no) 1638, (1, yes) 1542, (2, no) 1302, (2, yes) 856,
    shared 3: 186; coplanar overlapping pairs with at most one shared id per drop axis 936 / 331 / 243 (the tied
    normals of z = x + y and z = x all drop the lowest axis); fold-overs per unused slot of the higher face
    297 / 267 / 292 and per apex slot of the lower face 294 / 278 / 284."""
    vs, faces, pairs, n_deg = soups()
    assert n_deg > 0
    P = EX.points(vs)
    rows = faces.tolist()
    is_pair = set(map(tuple, pairs.tolist()))
    classes, coplanar, unused_hi, apex_lo = {}, [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for i, j in EX.candidates(vs, faces).tolist():
        fi, fj = rows[i], rows[j]
        if EX.degenerate(P, fi) or EX.degenerate(P, fj):
            continue
        shared, hit = len(set(fi) & set(fj)), (i, j) in is_pair
        key = (shared, hit) if shared < 3 else (3, True)
        classes[key] = classes.get(key, 0) + 1
        if hit and shared == 2:
            unused_hi[_slot_not_in(fj, fi)[0]] += 1
            apex_lo[_slot_not_in(fi, fj)[0]] += 1
        if hit and shared <= 1:                             # the in-plane branch of the segment test: proj and the drop axis
            ni, nj = EX.normal(P, fi), EX.normal(P, fj)
            if EX._cross(ni, nj) == (0, 0, 0) and EX._dot(ni, EX._sub(P[fj[0]], P[fi[0]])) == 0:
                mag = [abs(x) for x in ni]
                coplanar[mag.index(max(mag))] += 1
    print("classes", sorted(classes.items()), "coplanar", coplanar, "unused slot of the higher face", unused_hi,
          "apex slot of the lower face", apex_lo)
    assert set(classes) == {(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, True)}
    assert min(classes.values()) >= 30
    assert min(coplanar) >= 20
    assert min(unused_hi) >= 10 and min(apex_lo) >= 10


def test_the_soups_use_every_axis_map_winding_and_flatness():
    maps = IO.signed_axis_permutations()
    assert len(maps) == 48 and len({(tuple(p), tuple(s)) for p, s in maps}) == 48
    vs, faces, _, _ = soups()
    centres = IO.cluster_centres(125)
    local = vs.reshape(125, 7, 3) - centres[:, None, :]
    assert np.abs(local).max() <= 6 and np.abs(vs).max() <= 2 ** 10
    lo, hi = vs.reshape(125, 7, 3).min(1), vs.reshape(125, 7, 3).max(1)
    apart = ((lo[:, None] > hi[None]) | (lo[None] > hi[:, None])).any(2) | np.eye(125, dtype=bool)
    assert apart.all()                                                  # no box of one cluster touches another's
    assert (faces.reshape(125, 36) // 7 == np.arange(125)[:, None]).all()
    flat_axes = {int(np.flatnonzero((local[c] == 0).all(0))[0]) for c in range(125) if c % 5 == 2}
    assert flat_axes == {0, 1, 2}                                       # the soups in z = 0 end up in all three planes


@functools.lru_cache(maxsize=None)
def rotated():
    vs, faces = IO.rotated_soups(96)
    return vs, faces, IO.self_intersections(vs, faces)


def test_the_rotated_soups_depend_on_the_rounding_of_float64():
    """Seed 2024 (the first one tried): 536 marginal candidate pairs, 12 of them with a float64 verdict that the exact
    rational evaluation of the same float32 values reverses.  A verdict can only differ where a sign is in doubt, so the
    exact definition is asked about the marginal pairs alone."""
    vs, faces, want = rotated()
    assert vs.dtype == np.float32 and len(want) > 0
    assert len(want.marginal) >= 100
    P = EX.points(vs)
    is_pair = set(map(tuple, want.pairs.tolist()))
    rows = faces.tolist()
    differ = [(i, j) for i, j in want.marginal.tolist() if EX.crosses(P, rows[i], rows[j]) != ((i, j) in is_pair)]
    print("marginal", len(want.marginal), "float64 verdict differs from the exact one", differ)
    assert len(differ) >= 1
