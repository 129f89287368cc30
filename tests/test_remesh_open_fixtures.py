"""The premises of tests/remesh_open_fixtures.py, on the CPU: what tests/test_gpu_remesh_open.py compares the device with is
only worth something when a device with the mistake in question would give ANOTHER answer on these fixtures.  Each premise is
a condition on a fixture (if one fails, the fixture has to change, not the condition); the figures printed next to them are
those of the serial oracles."""
import random
from fractions import Fraction

import numpy as np
import pytest

import collapse_oracle as CO
import holes_oracle as HO
import remesh_oracle as RO
import remesh_open_fixtures as FX


# ---- the open meshes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FX.OPEN))
def test_open_fixture_premises(name):
    c = FX.open_case(name)
    V0 = c.vs.shape[0]
    assert RO.check_input(c.vs, c.faces)["n_nonmanifold"] == 0
    s_vs, s_faces, s_par, s_counts, s_long = c.split
    V1 = s_vs.shape[0]
    b0, b1 = FX.numpy_border(c.faces, V0), FX.numpy_border(s_faces, V1)
    assert s_long == 0 and np.array_equal(b1[:V0], b0)
    assert b1[V0:].sum() >= 20                             # the split inserts border vertices
    assert len(c.flip[1]) >= 3                             # the flip of the split mesh takes several rounds
    log = []
    with FX.altered(guard_log=log):
        again = RO.flip_edges(s_vs, s_faces)
    assert np.array_equal(again[0], c.flip[0]) and log.count(False) >= 20     # candidates that the guard ALONE refuses
    # a wrong border flag shows: inserted border vertices taken for interior ones, and every vertex taken for interior
    with FX.altered(border=lambda border, faces: {v for v in border if v < V0}):
        inserted_interior = RO.flip_edges(s_vs, s_faces)[0]
    with FX.altered(border=lambda border, faces: set()):
        all_interior = RO.flip_edges(s_vs, s_faces)[0]
    changed = (FX.faces_changed(inserted_interior, c.flip[0]), FX.faces_changed(all_interior, c.flip[0]))
    assert min(changed) >= 50
    assert np.array_equal(RO.flip_edges(s_vs, s_faces)[0], c.flip[0])          # and the oracle is itself again
    # the collapse of the split mesh does something, keeps the border vertices and the loops
    c_vs, c_faces, ids, merged, c_counts, c_short = c.collapse
    assert len(c_counts) >= 3 and c_vs.shape[0] < V1 and b1[ids].sum() == b1.sum()
    assert np.array_equal(FX.numpy_border(c_faces, c_vs.shape[0]), b1[ids])
    loops = [len(HO.boundary_loops(f)) for f in (c.faces, s_faces, c.flip[0], c_faces, c.flip2[0])]
    assert len(set(loops)) == 1 and loops[0] == {"wavy12": 1, "holed20x12": 2}[name]
    print(name, "V", V0, "->", V1, "F", c.faces.shape[0], "->", s_faces.shape[0], "split rounds", len(s_counts), "border", int(b0.sum()),
          "->", int(b1.sum()), "inserted on the border", int(b1[V0:].sum()), "flips", c.flip[1], "deviation", c.flip[2], "->", c.flip[3],
          "guard refusals", log.count(False), "/", len(log), "faces changed by the altered oracles", changed, "collapse rounds",
          len(c_counts), "V ->", c_vs.shape[0])
    # the figures of the prototype
    want = {"wavy12": (169, 459, 288, 846, 7, 48, 70, 22), "holed20x12": (206, 926, 379, 1776, 11, 37, 80, 43)}[name]
    assert (V0, V1, c.faces.shape[0], s_faces.shape[0], len(s_counts), b0.sum(), b1.sum(), b1[V0:].sum()) == want
    if name == "holed20x12":
        assert 3 * s_faces.shape[0] == 5328                # 21 workgroups of 256; the plan's buffers grow on the way


@pytest.mark.parametrize("name", sorted(FX.OPEN))
def test_inserted_border_vertices_come_from_border_edges(name):
    """The rule the device test holds the plan's carried flags to, checked on the oracle first: an inserted vertex is on the
    border exactly when the edge it split had one face."""
    c = FX.open_case(name)
    vs, faces = c.vs, c.faces
    thr2 = RO.split_threshold(c.target)
    while True:
        table = RO.edge_table(faces)[0]
        V = vs.shape[0]
        new_vs, new_faces, ends, _ = RO.split_round(vs, faces, thr2)
        if not ends:
            break
        border = FX.numpy_border(new_faces, new_vs.shape[0])
        for s, (lo, hi) in enumerate(ends):
            assert border[V + s] == (len(table[(lo, hi)]) == 1)
        vs, faces = new_vs, new_faces
    assert np.array_equal(faces, c.split[1])


# ---- the guard at exactly zero ---------------------------------------------------------------------------------------------
def _exact_dots(vs, a, b, c, d):
    P = [[Fraction(float(x)) for x in p] for p in vs]
    sub = lambda p, q: [P[p][i] - P[q][i] for i in range(3)]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    n = lambda p, q, r: cross(sub(q, p), sub(r, p))
    old, new = (n(a, b, c), n(b, a, d)), (n(a, d, c), n(d, b, c))
    return [sum(x * y for x, y in zip(u, v)) for u in new for v in old]


@pytest.mark.parametrize("name", ["fan8_on_chord", "fan8_right_angle"])
def test_flip_guard_tie_premises(name):
    vs, faces, j = getattr(FX, name)()
    RO.check_input(vs, faces)
    before, after = 1 + (j - 2) % 8, 1 + j % 8
    dots = _exact_dots(vs, 0, j, after, before)
    assert min(dots) == 0 and max(dots) >= 0               # exactly zero, none negative: only the strictness decides
    old = (RO._normal(vs, 0, j, after), RO._normal(vs, j, 0, before))
    new = (RO._normal(vs, 0, before, after), RO._normal(vs, before, j, after))
    assert sorted(RO._dot(n, o) for n in new for o in old) == sorted(float(x) for x in dots)  # float64 sees the same numbers
    if name == "fan8_right_angle":
        assert max(dots) > 0 and not FX.zero_area_faces(vs, [(0, before, after), (before, j, after)])
    else:
        assert FX.zero_area_faces(vs, [(before, j, after)]) == [0]
    cands = RO.flip_candidates(vs, faces)
    assert (0, j) not in cands and len(cands) >= 4          # the oracle refuses the spoke ...
    want = RO.flip_edges(vs, faces)
    with FX.altered(zero_passes=True):
        loose_cands = RO.flip_candidates(vs, faces)
        loose = RO.flip_edges(vs, faces)
    # ... which would win the first round: a guard with >= gives other faces
    assert max(loose_cands, key=lambda e: loose_cands[e][0]) == (0, j)
    assert FX.faces_changed(want[0], loose[0]) > 0
    assert not FX.zero_area_faces(vs, want[0])
    if name == "fan8_on_chord":
        assert FX.zero_area_faces(vs, loose[0])             # and there it makes a face of zero area


def test_collapse_guard_tie_premises():
    vs, faces = FX.fan7_collinear()
    RO.check_input(vs, faces)
    lo2, thr2 = CO.collapse_threshold(FX.GUARD_TIE_TARGET), RO.split_threshold(FX.GUARD_TIE_TARGET)
    assert min(RO.edge_table(faces)[0], key=lambda e: RO.len2(vs, *e)) == (0, 1)
    assert RO._dot(RO._normal(vs, 0, 2, 3), RO._normal(vs, 1, 2, 3)) == 0.0
    assert (0, 1) not in CO.collapse_candidates(vs, faces, lo2, thr2)
    with FX.altered(zero_passes=True):
        loose_cands = CO.collapse_candidates(vs, faces, lo2, thr2)
        loose = CO.collapse_short_edges(vs, faces, FX.GUARD_TIE_TARGET)
    assert max(loose_cands, key=lambda e: loose_cands[e][0]) == (0, 1)
    want = CO.collapse_short_edges(vs, faces, FX.GUARD_TIE_TARGET)
    assert want[4] and not np.array_equal(want[1], loose[1])
    assert not FX.zero_area_faces(want[0], want[1]) and FX.zero_area_faces(loose[0], loose[1])


# ---- thresholds within one ulp ---------------------------------------------------------------------------------------------
def test_round_f32_is_round_to_nearest_even():
    rnd = random.Random(3)
    for _ in range(2000):
        x = rnd.uniform(-4, 4) * 2.0 ** rnd.randint(-130, 20)
        assert FX.round_f32(Fraction(x)).view(np.uint32) == np.float32(x).view(np.uint32), x    # one rounding, double -> float32
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert FX.round_f32(one + ulp / 2) == np.float32(1.0)                      # a tie goes to the even neighbour
    assert FX.round_f32(one + ulp + ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)
    assert FX.round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.float32(1.0) + np.float32(2.0 ** -23)   # no double rounding
    vs = np.array([[1, 2, 3], [4, -2, 9]], np.float32)
    assert FX.len2_fused(vs, 0, 1) == RO.len2(vs, 0, 1) == 61                  # exact operands: nothing to round


def _edges_len2(vs, faces):
    return {e: (RO.len2(vs, *e), len(hs)) for e, hs in RO.edge_table(faces)[0].items()}


@pytest.mark.parametrize("name", sorted(FX.TIE_SOUPS))
def test_tie_soup_premises(name):
    vs, faces, info = FX.tie_soup(name)
    RO.check_input(vs, faces)
    thr, cmp = info.threshold, info.compare
    lo2, thr2 = CO.collapse_threshold(FX.TIE_TARGET), RO.split_threshold(FX.TIE_TARGET)
    assert 100 <= info.n_components and 100 <= faces.shape[0] <= 600
    tied = {tuple(e) for e in info.edges.tolist()}
    lens = _edges_len2(vs, faces)
    for i, e in enumerate(info.edges.tolist()):
        assert RO.len2(vs, *e) == info.unfused[i] and FX.len2_fused(vs, *e) == info.fused[i]
        assert (tuple(e) in lens) == (name != "guard")      # "guard": the tied pair is the edge the collapse would create
        assert abs(RO.bits(info.unfused[i]) - RO.bits(thr)) <= 1
    discordant = cmp(info.unfused, thr) != cmp(info.fused, thr)
    exact = info.unfused == thr
    print(name, "components", info.n_components, "discordant", int(discordant.sum()), "len2 == threshold", int(exact.sum()),
          "decided", int(cmp(info.unfused, thr).sum()), "unfused,", int(cmp(info.fused, thr).sum()), "fused")
    assert discordant.sum() >= 64 and exact.sum() >= 8 and cmp(info.unfused, thr).any() and not cmp(info.unfused, thr).all()
    others = {e: l for e, l in lens.items() if e not in tied}
    if name == "split":                                    # the other two edges are clearly not long
        assert all(l2 < 0.5 * thr2 for l2, _ in others.values())
        want = RO.split_long_edges(vs, faces, FX.TIE_TARGET, max_rounds=1)
        with FX.altered(fused=True):
            fused = RO.split_long_edges(vs, faces, FX.TIE_TARGET, max_rounds=1)
        assert want[3] == [int((info.unfused > thr).sum())] and fused[3] == [int((info.fused > thr).sum())]
        assert want[2][vs.shape[0]:].tolist() == [e for e, u in zip(info.edges.tolist(), info.unfused) if u > thr]
        assert want[2][vs.shape[0]:].tolist() != fused[2][vs.shape[0]:].tolist()
    else:
        # the tied edge decides alone: no other interior edge is near lo2, no other future edge is near thr2
        spokes = {e: l2 for e, (l2, k) in others.items() if k == 2}
        if name == "short":
            assert all(l2 > 1.2 * lo2 for l2 in spokes.values())
        else:
            short = [e for e, l2 in spokes.items() if l2 < lo2]
            assert len(short) == info.n_components and all(spokes[e] < 0.9 * lo2 for e in short)
            assert all(l2 > 1.2 * lo2 for e, l2 in spokes.items() if e not in short)
        assert all(l2 < 0.9 * thr2 for l2, _ in others.values())
        decides = (lambda l2: l2 < thr) if name == "short" else (lambda l2: not l2 > thr)
        want = CO.collapse_short_edges(vs, faces, FX.TIE_TARGET)
        with FX.altered(fused=True):
            fused = CO.collapse_short_edges(vs, faces, FX.TIE_TARGET)
        assert want[4] == [sum(bool(decides(u)) for u in info.unfused)] and fused[4] == [sum(bool(decides(u)) for u in info.fused)]
        removed = lambda r: sorted(set(range(vs.shape[0])) - set(r[2].tolist()))
        apex = lambda keep: [5 * i + 4 for i, u in enumerate(keep) if decides(u)]
        assert removed(want) == apex(info.unfused) and removed(fused) == apex(info.fused) and removed(want) != removed(fused)
    assert RO.len2 is not FX.len2_fused and CO.len2 is RO.len2                 # the oracles are themselves again
