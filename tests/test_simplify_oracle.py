"""The premises of tests/simplify_oracle.py, the numpy restatement tests/test_gpu_simplify.py holds the device to, on the
fixtures of tests/simplify_fixtures.py: what every result must satisfy, the hand-computed cases, and the reference's own
hierarchy of the 258-vertex sphere (golden g3) as the bar for the summed cluster quadric error."""
import numpy as np
import pytest

import golden_util as GU
import remesh_oracle as RO
import simplify_fixtures as SF
import simplify_oracle as SO


def _border(faces):
    return sorted({v for e, n in SF.edge_counts(faces).items() if n == 1 for v in e})


@pytest.mark.parametrize("quadrics", ["own", "sum"])
@pytest.mark.parametrize("name,ratio", SF.CASES)
def test_premises_on_every_fixture(name, ratio, quadrics):
    c = SF.case(name, ratio, quadrics)
    V = c.in_vs.shape[0]
    assert c.reached == (c.vs.shape[0] == c.target) and (c.reached or name == "foldover")
    assert c.vs.shape[0] == V - sum(w for _, _, w in c.counts) and all(a <= n and w <= a and w >= 1 for n, a, w in c.counts)
    # the same kind of surface: every edge with the face counts of a manifold, Euler characteristic and border kept
    counts_in, counts_out = SF.edge_counts(c.in_faces), SF.edge_counts(c.faces)
    assert set(counts_out.values()) <= ({1, 2} if name in SF.OPEN else {2})
    assert RO.check_input(c.vs, c.faces)["n_misoriented"] == 0
    assert SF.euler(c.vs, c.faces) == SF.euler(c.in_vs, c.in_faces)
    assert sum(n == 1 for n in counts_out.values()) == sum(n == 1 for n in counts_in.values())
    # the maps
    assert np.array_equal(c.coarse_of[c.vertex_ids], np.arange(c.vs.shape[0])) and (np.diff(c.vertex_ids) > 0).all()
    assert c.coarse_of.shape == (V,) and set(c.coarse_of.tolist()) == set(range(c.vs.shape[0]))
    b_in = _border(c.in_faces)
    if name in SF.OPEN:                                    # border vertices survive where they were, bit for bit
        assert b_in and set(b_in) <= set(c.vertex_ids.tolist())
        assert c.vs[c.coarse_of[b_in]].tobytes() == c.in_vs[b_in].tobytes()
        assert sorted(c.coarse_of[b_in].tolist()) == _border(c.faces)
    else:                                                  # closed: the survivor of a cluster is its smallest member
        first = np.full(c.vs.shape[0], V)
        np.minimum.at(first, c.coarse_of, np.arange(V))
        assert not b_in and np.array_equal(first, c.vertex_ids)
    # no face normal reverses -- checked on the faces themselves, not through the guard: a surviving face keeps the side of
    # the input face it was (same slot order: survivors are compacted stably)
    alive = np.array([len({int(v) for v in c.coarse_of[t]}) == 3 for t in c.in_faces])
    assert np.array_equal(c.coarse_of[c.in_faces[alive]], c.faces)
    n_in, n_out = SO.face_normals(c.in_vs, c.in_faces[alive]), SO.face_normals(c.vs, c.faces)
    if name in ("foldover", "foldover_mid", "flat_grid"):
        assert (n_out[:, 2] > 0).all() and (n_in[:, 2] > 0).all()
    elif name in ("sphere258", "sphere66", "valence3"):
        assert ((n_out * c.vs[c.faces].mean(1)).sum(1) > 0).all()       # outward
    else:                                                  # a face still looks the way the input face it was looked
        cos = (n_in * n_out).sum(1) / (np.linalg.norm(n_in, axis=1) * np.linalg.norm(n_out, axis=1))
        print(name, ratio, quadrics, "smallest cosine between a face and what it became", float(cos.min()))
        assert (cos > 0).all()


def test_tetrahedron_has_no_legal_collapse():
    vs, faces = RO.tetrahedron()
    legal, refused = SO.candidates(vs, faces, SO.vertex_quadrics(vs, faces))
    assert legal == {} and refused == 6                    # every edge is eligible; the valence floors refuse all six
    out = SO.simplify(vs, faces, 3)
    assert out[0].tobytes() == vs.tobytes() and np.array_equal(out[1], faces) and out[4] == [] and not out[5] and out[6] == 6


def test_edges_round_a_valence_three_vertex_fail_the_link_condition():
    vs, faces = SF.mesh("valence3")
    table, _ = RO.edge_table(faces)
    val, border = RO.valences(faces)
    ring = {}
    for a, b in table:
        ring.setdefault(a, set()).add(b)
        ring.setdefault(b, set()).add(a)
    assert val[18] == 3 and not border
    a, b, c = sorted(ring[18])
    legal, refused = SO.candidates(vs, faces, SO.vertex_quadrics(vs, faces))
    unguarded, _ = SO.candidates(vs, faces, SO.vertex_quadrics(vs, faces), guard=False)
    around = [(a, b), (a, c), (b, c)]
    for e in around:                                       # three shared neighbours: 18, the third corner, the vertex across
        assert len(ring[e[0]] & ring[e[1]]) == 3 and e not in legal and e not in unguarded
    assert refused >= 3 and all((v, 18) in legal for v in (a, b, c))      # the vertex itself may go: two shared neighbours
    assert all(len(ring[e[0]] & ring[e[1]]) == 2 for e in legal)


def test_the_guard_refuses_the_cheapest_edge_and_the_next_is_taken():
    vs, faces = SF.mesh("foldover")
    assert (SO.face_normals(vs, faces)[:, 2] > 0).all()
    Q = SO.vertex_quadrics(vs, faces)
    off, _ = SO.candidates(vs, faces, Q, guard=False)
    on, refused = SO.candidates(vs, faces, Q, guard=True)
    top = max(off, key=lambda e: off[e][0])
    assert top == (5, 11) and top not in on and refused == len(off) - len(on) == 3
    assert {e: on[e][:4] for e in on} == {e: off[e][:4] for e in on}       # the guard changes nothing else
    best = max(on, key=lambda e: on[e][0])
    g_off = SO.simplify(vs, faces, 24, guard=False)
    g_on = SO.simplify(vs, faces, 24)
    assert g_off[4] == [(38, 1, 1)] and g_on[4] == [(35, 1, 1)]
    assert int(np.setdiff1d(np.arange(25), g_off[2])[0]) == 11 and int(np.setdiff1d(np.arange(25), g_on[2])[0]) == on[best][2]
    assert (SO.face_normals(g_off[0], g_off[1])[:, 2] < 0).any()           # without the guard a face IS reversed
    assert (SO.face_normals(g_on[0], g_on[1])[:, 2] > 0).all()


def test_the_guard_refuses_a_midpoint_collapse_that_reverses_a_face():
    """Both ends of the cheapest edge {19, 26} are interior: 19 is kept and moves to the float32 midpoint, 26 goes."""
    vs, faces = SF.mesh("foldover_mid")
    assert (SO.face_normals(vs, faces)[:, 2] > 0).all()
    border = set(_border(faces))
    Q = SO.vertex_quadrics(vs, faces)
    off, _ = SO.candidates(vs, faces, Q, guard=False)
    on, refused = SO.candidates(vs, faces, Q, guard=True)
    top = max(off, key=lambda e: off[e][0])
    key, k, r, moves, pos, _, cost = off[top]
    assert top == (19, 26) and not {19, 26} & border and (k, r, moves, cost) == (19, 26, True, 0.0)
    assert [float(x) for x in pos] == [float((vs[19][i] + vs[26][i]) * np.float32(0.5)) for i in range(3)]
    assert top not in on and refused == len(off) - len(on) == 7
    best = max(on, key=lambda e: on[e][0])
    g_off = SO.simplify(vs, faces, 35, guard=False)
    g_on = SO.simplify(vs, faces, 35)
    assert g_off[4] == [(63, 1, 1)] and g_on[4] == [(56, 1, 1)]
    assert int(np.setdiff1d(np.arange(36), g_off[2])[0]) == 26 and int(np.setdiff1d(np.arange(36), g_on[2])[0]) == on[best][2]
    assert g_off[0][19].tobytes() == np.array(pos, np.float32).tobytes()   # 26 is gone, 19 sits at the midpoint
    assert (SO.face_normals(g_off[0], g_off[1])[:, 2] < 0).any()           # without the guard a face IS reversed
    assert (SO.face_normals(g_on[0], g_on[1])[:, 2] > 0).all()


def test_flat_integer_grid_costs_are_exactly_zero_and_the_hash_orders():
    vs, faces = SF.mesh("flat_grid")
    Q = SO.vertex_quadrics(vs, faces)
    assert np.array_equal(Q, np.round(Q)) and (Q[:, [0, 1, 2, 3, 4, 5, 6]] == 0).all()
    legal, refused = SO.candidates(vs, faces, Q)
    _, rank = RO.edge_table(faces)
    assert legal and refused == 0 and all(c[6] == 0.0 and c[0] >> 32 == 0xFFFFFFFF for c in legal.values())
    assert all(c[0] & 0xFFFFFFFF == RO.hash32(rank[e]) for e, c in legal.items())
    out = SO.simplify_round(vs, faces, Q, 1)
    gone = int(np.setdiff1d(np.arange(vs.shape[0]), out[3])[0])
    assert out[5] == (len(legal), 1, 1) and gone == legal[max(legal, key=lambda e: RO.hash32(rank[e]))][2]


def test_costs_equal_in_float32_are_ordered_by_the_hash_not_by_float64():
    """The 66-vertex sphere: symmetric edges have costs that differ only in the last bits of the float64.  Among the winners
    of the first round at ratio 0.6 is one that beat an edge of its neighbourhood that is cheaper in float64, on the hash alone."""
    vs, faces = SF.mesh("sphere66")
    Q = SO.vertex_quadrics(vs, faces)
    legal, _ = SO.candidates(vs, faces, Q)
    need = 66 - int(66 * 0.6)
    admitted = sorted(legal, key=lambda e: legal[e][0], reverse=True)[:need]
    out = SO.simplify_round(vs, faces, Q, need)
    removed = set(np.setdiff1d(np.arange(66), out[3]).tolist())
    winners = [e for e in admitted if legal[e][2] in removed and out[4][legal[e][2]] == out[4][legal[e][1]]]
    assert len(winners) == out[5][2] >= 1
    shown = [(w, o) for w in winners for o in admitted
             if o != w and legal[o][5] & legal[w][5] and legal[o][6] < legal[w][6]]
    assert shown, "no winner beat a float64-cheaper neighbour"
    for w, o in shown:
        assert np.float32(legal[w][6]) == np.float32(legal[o][6]) and legal[w][6] != legal[o][6]
        assert legal[w][0] & 0xFFFFFFFF > legal[o][0] & 0xFFFFFFFF


def _levels(vs0, faces0, targets, quadrics):
    vs, faces, comp, errs = vs0, faces0, np.arange(vs0.shape[0]), []
    for t in targets:
        out = SO.simplify(vs, faces, t, quadrics=quadrics)
        assert out[5]
        vs, faces, comp = out[0], out[1], out[3][comp]
        errs.append(SO.cluster_quadric_error(vs0, faces0, comp, vs))
    return errs


@pytest.mark.parametrize("quadrics", ["own", "sum"])
def test_no_more_quadric_error_than_the_references_own_hierarchy(quadrics):
    """Golden g3 holds the hierarchy the reference's ``Mesh.simplification`` built of the 258-vertex sphere.  The oracle, run on
    the same sphere to the same level-1 and level-2 vertex counts, must not exceed the reference's summed cluster quadric
    error (tests/test_gpu_parity.py::_cluster_quadric_error, restated in numpy) at either level.  Measured: 5.926 and 23.72
    with "own", 5.848 and 20.96 with "sum", against the reference's 13.49 and 56.94."""
    g3 = GU.load("g3_mgcn.npz")
    vs0, faces0 = g3["poss/0"].astype(np.float32), SF.mesh("sphere258")[1]
    assert np.abs(vs0 - SF.mesh("sphere258")[0]).max() < 1e-6
    targets = [g3["poss/1"].shape[0], g3["poss/2"].shape[0]]
    assert targets == [154, 92]
    comp, ref = np.arange(258), []
    for l in range(2):
        comp = g3[f"pool_hash/{l}"][:, 1][comp]
        ref.append(SO.cluster_quadric_error(vs0, faces0, comp, g3[f"poss/{l + 1}"]))
    got = _levels(vs0, faces0, targets, quadrics)
    print("summed cluster quadric error per level: oracle", quadrics, got, "reference", ref)
    assert all(g <= r for g, r in zip(got, ref))
