"""The premises of tests/simplify_oracle.py, the numpy restatement tests/test_gpu_simplify.py holds the device to, on the
fixtures of tests/simplify_fixtures.py: what every result must satisfy, the hand-computed cases, and the reference's own
hierarchy of the 258-vertex sphere (golden g3) as the bar for the summed cluster quadric error."""
import itertools

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


# ---- the edge fixtures of tests/test_gpu_simplify_edges.py: what each of them reaches, from the oracle ------------------------
def _rings(faces):
    ring = {}
    for a, b in RO.edge_table(faces)[0]:
        ring.setdefault(a, set()).add(b)
        ring.setdefault(b, set()).add(a)
    return ring


def _legal_but_for_the_fan(faces, e):
    """``c != d``, the link count and the three valence floors of edge ``e``, by hand (the guard and the cost are not asked)."""
    table, _ = RO.edge_table(faces)
    val, border = RO.valences(faces)
    ring = _rings(faces)
    a, b = e
    k = a if a in border else (b if b in border else min(a, b))
    r = b if k == a else a
    floor = lambda v: 2 if v in border else 3
    c, d = (int(faces[h // 3][(h % 3 + 2) % 3]) for h in table[e])
    return (len(table[e]) == 2 and not (a in border and b in border) and c != d and len(ring[r] & ring[k]) == 2
            and val[c] - 1 >= floor(c) and val[d] - 1 >= floor(d) and val[k] + val[r] - 4 >= floor(k))


@pytest.mark.parametrize("name,ratio,n_edges,eligible,fans_in,first,rounds,refused", [
    ("touch_closed", 0.6, 8, [(0, 18), (0, 19), (0, 20), (0, 21), (0, 83), (0, 84), (0, 85), (0, 86)], [4, 4], (376, 53, 7), 12, 14),
    ("touch_open", 0.7, 6, [(0, 6), (0, 30)], [2, 2], (74, 15, 2), 11, 4),
    ("touch_mixed", 0.6, 7, [(0, 18), (0, 19), (0, 20), (0, 21), (0, 70)], [4, 2], (206, 33, 6), 12, 8)])
def test_no_edge_at_a_vertex_where_two_fans_touch_is_legal(name, ratio, n_edges, eligible, fans_in, first, rounds, refused,
                                                           monkeypatch):
    """Every eligible edge at the shared vertex would be legal but for "the faces at r or at k are not one fan"; the vertex
    survives with both fans."""
    vs, faces = SF.mesh(name)
    assert RO.check_input(vs, faces)["n_nonmanifold"] == 0
    table, _ = RO.edge_table(faces)
    val, border = RO.valences(faces)
    at = sorted(e for e in table if SF.TOUCH in e)
    assert len(at) == n_edges == val[SF.TOUCH] and SF.fans(faces, SF.TOUCH) == fans_in
    assert sorted(e for e in at if len(table[e]) == 2 and not (e[0] in border and e[1] in border)) == eligible
    assert (SF.TOUCH in border) == (name != "touch_closed")
    Q = SO.vertex_quadrics(vs, faces)
    legal, n_refused = SO.candidates(vs, faces, Q)
    assert not [e for e in at if e in legal] and n_refused == len(eligible)
    assert all(_legal_but_for_the_fan(faces, e) for e in eligible)             # by hand: c != d, the link, the floors
    monkeypatch.setattr(SO, "_one_fan", lambda rot: True)                      # and by the oracle without the fan clause:
    anyway, none = SO.candidates(vs, faces, Q)                                 # the guard and the cost pass too
    monkeypatch.undo()
    assert none == 0 and set(anyway) == set(legal) | set(eligible)
    if name != "touch_closed":                                                 # the shared vertex is a border vertex: kept
        assert all(anyway[e][1] == SF.TOUCH and not anyway[e][3] for e in eligible)
    c = SF.case(name, ratio, "own")
    assert c.reached and c.counts[0] == first and len(c.counts) == rounds and c.refused == refused
    assert c.vertex_ids[0] == SF.TOUCH and (c.coarse_of == 0).sum() == 1       # neither removed nor merged into
    assert len(SF.fans(c.faces, 0)) == 2 and c.vs[0].tobytes() == vs[SF.TOUCH].tobytes()
    assert set(SF.edge_counts(c.faces).values()) == ({2} if name == "touch_closed" else {1, 2})


def test_a_face_without_area_gives_no_quadric_and_fails_the_guard_at_zero():
    vs, faces = SF.mesh("flat_face")
    v, x, y = SF.FLAT_FACE
    flat = [f for f, t in enumerate(faces.tolist()) if set(t) == {v, x, y}]
    nrm = SO.face_normals(vs, faces)
    assert len(flat) == 1 and len({vs[u].tobytes() for u in (v, x, y)}) == 3
    assert np.nonzero((nrm * nrm).sum(1) == 0)[0].tolist() == flat and (nrm[:, 2] >= 0).all() and (nrm[:, 2] > 0).sum() == 49
    assert SO.face_quadric(vs, faces[flat[0]]) is None
    Q = SO.vertex_quadrics(vs, faces)
    rest = np.delete(faces, flat[0], 0)
    assert Q.tobytes() == SO.vertex_quadrics(vs, rest).tobytes() and np.isfinite(Q).all()     # "contributes nothing"
    on, r_on = SO.candidates(vs, faces, Q)
    off, r_off = SO.candidates(vs, faces, Q, guard=False)
    by_guard = sorted(set(off) - set(on))
    assert (len(on), len(off), r_off, r_on) == (50, 63, 0, 13) and all(set(e) & {v, x, y} for e in by_guard)
    assert (13, 14) in on and (7, 14) in on                # the two edges whose collapse deletes the flat face
    # the dot product that refuses is exactly 0, not negative: n_old of the flat face is the zero vector
    zero = 0
    for e in by_guard:
        _, k, r, moves, pos, _, _ = off[e]
        for w, other in ((r, k), (k, r)):
            for t in faces.tolist():
                if w in t and other not in t and (w != k or moves):
                    i = t.index(w)
                    d = RO._dot(SO._normal_at(vs[w], vs, t[(i + 1) % 3], t[(i + 2) % 3]),
                                SO._normal_at(pos, vs, t[(i + 1) % 3], t[(i + 2) % 3]))
                    zero += d == 0.0
    assert zero >= 1
    c = SF.case("flat_face", 0.6, "own")
    n_out = SO.face_normals(c.vs, c.faces)
    assert c.reached and len(c.counts) == 14 and ((n_out * n_out).sum(1) > 0).all()
    assert len(SF.case("flat_face", 0.6, "sum").counts) == 11


UNIT = [(192, 27, 5), (177, 22, 3), (168, 19, 3)]
CLAMPED = [(192, 27, 3), (183, 24, 4), (171, 20, 1)]


@pytest.mark.parametrize("k,first,rounds,refused", [(60, UNIT, 9, 0), (100, CLAMPED, 17, 30), (-70, UNIT, 9, 0),
                                                    (-80, CLAMPED, 17, 30), (-140, CLAMPED, 17, 30)])
def test_the_float32_end_of_the_priority(k, first, rounds, refused):
    """What each scale of the 66-vertex sphere does to the first round's 192 costs and to the coordinates."""
    tiny = float(np.finfo(np.float32).tiny)
    vs, faces = SF.mesh(f"sphere66_2^{k}")
    unit = SF.mesh("sphere66")[0]
    sub = (vs != 0) & (np.abs(vs) < tiny)
    assert np.isfinite(vs).all() and ((vs == 0) == (unit == 0)).all()
    Q = SO.vertex_quadrics(vs, faces)
    legal, _ = SO.candidates(vs, faces, Q)
    cost = np.array([c[6] for c in legal.values()])
    with np.errstate(all="ignore"):
        c32 = cost.astype(np.float32)
    high = {c[0] >> 32 for c in legal.values()}
    assert cost.shape == (192,) and np.isfinite(Q).all() and (Q != 0).any(1).all() and (cost > 0).all()
    n_clamped, n_sub, n_zero = int((cost > SO.F32_MAX).sum()), int(((c32 != 0) & (c32 < tiny)).sum()), int((c32 == 0).sum())
    print(k, "costs from", cost.min(), "to", cost.max(), "clamped", n_clamped, "subnormal", n_sub, "zero", n_zero,
          "subnormal coordinates", int(sub.sum()))
    if k == 60:
        assert (n_clamped, n_sub, n_zero, int(sub.sum())) == (0, 0, 0, 0) and len(high) > 1
    elif k == 100:
        assert n_clamped == 192 and 9.5e58 < cost.min() and cost.max() < 2.2e60
        assert high == {RO.MASK - RO.bits(np.float32(SO.F32_MAX))}               # one high word: the hash alone orders
    elif k == -70:
        assert (n_clamped, n_sub, n_zero, int(sub.sum())) == (0, 192, 0, 0) and len(high) > 1
    elif k == -80:
        assert (n_clamped, n_sub, n_zero, int(sub.sum())) == (0, 0, 192, 0) and high == {RO.MASK}
    else:
        assert (n_zero, int(sub.sum()), vs.size) == (192, 150, 198) and high == {RO.MASK}
        mids = np.array([c[4] for c in legal.values() if c[3]], np.float32)      # halving a subnormal: ties go to even
        exact = np.array([[(float(vs[e[0]][i]) + float(vs[e[1]][i])) / 2 for i in range(3)] for e, c in legal.items() if c[3]])
        assert (mids.astype(np.float64) != exact).any()
    for q in ("own", "sum"):
        c = SF.case(f"sphere66_2^{k}", 0.6, q)
        unit_like = first is UNIT
        want3 = first if q == "own" or not unit_like else first[:2] + [(168, 19, 5)]
        assert c.reached and c.refused == refused and c.counts[:3] == want3
        assert len(c.counts) == (rounds if q == "own" or not unit_like else 10)
        # the rounds are those of the unit sphere, or -- where every cost is one float32 -- those of 2^100: flushing the
        # subnormal costs of 2^-70 to zero would give the second kind, which differs in its first round
        same = SF.case("sphere66" if unit_like else "sphere66_2^100", 0.6, q)
        assert c.counts == same.counts and np.array_equal(c.faces, same.faces) and np.array_equal(c.coarse_of, same.coarse_of)
        if unit_like:                                        # no coordinate rounds: the scaled result, bit for bit
            assert (same.vs * np.float32(2.0 ** k)).tobytes() == c.vs.tobytes()


def test_hub_sphere_prices_and_bids_round_two_poles_of_valence_80():
    vs, faces = SF.mesh("hub_sphere")
    val, border = RO.valences(faces)
    assert vs.shape[0] == 162 and not border and [val[0], val[161]] == [80, 80] and max(val[v] for v in range(1, 161)) == 5
    assert SF.euler(vs, faces) == 2 and ((SO.face_normals(vs, faces) * vs[faces].mean(1)).sum(1) > 0).all()
    legal, refused = SO.candidates(vs, faces, SO.vertex_quadrics(vs, faces))
    # the north pole is the kept end of its 80 edges (the fan of k: a walk of 80 faces), the south pole the removed end of its
    # 80 (the fan of r: 80 faces, and one link search per ring vertex)
    assert len(legal) == 480 and refused == 0
    assert sum(1 for c in legal.values() if c[1] == 0) == 80 and sum(1 for c in legal.values() if c[2] == 161) == 80
    assert sum(1 for c in legal.values() if {0, 161} & c[5]) == 480 and max(len(c[5]) for c in legal.values()) == 83
    c = SF.case("hub_sphere", 0.6, "sum")
    after, _ = RO.valences(c.faces)
    assert c.reached and len(c.counts) == 50 and c.counts[0] == (480, 65, 1) and max(w for _, _, w in c.counts) == 2
    assert (c.coarse_of == c.coarse_of[0]).sum() == 1 and (c.coarse_of == c.coarse_of[161]).sum() == 1    # no pole is merged
    assert max(after.values()) == 48 and [after[int(c.coarse_of[p])] for p in (0, 161)] == [47, 48]


@pytest.mark.parametrize("quadrics", ["own", "sum"])
def test_hub_disc_collapses_into_a_centre_of_valence_80(quadrics):
    vs, faces = SF.mesh("hub_disc")
    centre = SF.DISC_CENTRE
    val, border = RO.valences(faces)
    assert vs.shape[0] == 161 and val[centre] == 80 and border == set(range(80)) and (vs[:, 2] == 2).all()
    assert (SO.face_normals(vs, faces)[:, 2] > 0).all()
    hub = []
    for n, (_, _, legal, winners, val) in enumerate(itertools.islice(SF.trace("hub_disc", int(161 * SF.DISC_RATIO), quadrics), 3)):
        assert all(c[6] == 0.0 and c[0] >> 32 == RO.MASK for c in legal.values())
        hub += [(n, e, val[legal[e][1]] + val[legal[e][2]] - 4, len(legal[e][5])) for e in winners
                if legal[e][1] == centre and legal[e][3]]
    print("collapses that keep the centre: (round, edge, val_new, footprint)", hub)
    assert hub[0] == (0, (80, 156), 81, 83) and len(hub) == 3 and all(h[2] > 64 and h[3] > 64 for h in hub[:3])
    c = SF.case("hub_disc", SF.DISC_RATIO, quadrics)
    assert c.reached and c.counts[:3] == [(320, 33, 1), (121, 32, 1), (104, 31, 1)] and len(c.counts) == 33 and c.refused == 146
    assert c.vs[c.coarse_of[centre]].tobytes() != vs[centre].tobytes() and (c.coarse_of == c.coarse_of[centre]).sum() > 3


@pytest.mark.parametrize("quadrics,third,rounds_to_5", [("own", (168, 20, 3), 37), ("sum", (168, 20, 5), 38)])
def test_vertices_no_face_uses_count_in_the_budget_and_pass_through(quadrics, third, rounds_to_5):
    vs, faces = SF.mesh("unused3")
    assert vs.shape[0] == 69 and sorted(set(range(69)) - set(faces.reshape(-1).tolist())) == list(SF.UNUSED)
    assert RO.check_input(vs, faces)["n_degenerate"] == 0
    c = SF.case("unused3", 0.6, quadrics)
    assert c.target == 41 and c.reached and len(c.counts) == 10 and c.counts[:3] == [(192, 28, 5), (177, 23, 3), third]
    assert c.counts[0][1] == 69 - 41                         # need counts the unused three: 28, not the 66-vertex sphere's 27
    assert (np.diff(c.vertex_ids) > 0).all() and set(SF.UNUSED) <= set(c.vertex_ids.tolist())
    for u in SF.UNUSED:
        assert c.vertex_ids[c.coarse_of[u]] == u and (c.coarse_of == c.coarse_of[u]).sum() == 1
        assert c.vs[c.coarse_of[u]].tobytes() == vs[u].tobytes() and not (c.faces == c.coarse_of[u]).any()
    low = SF.run("unused3", 5, quadrics)
    assert not low.reached and low.vs.shape[0] == 7 and low.refused == 6 and low.counts[0] == (192, 64, 5)
    assert len(low.counts) == rounds_to_5 and set(SF.UNUSED) <= set(low.vertex_ids.tolist()) and low.faces.shape[0] == 4


def test_round_cap_and_the_ends_of_the_budget():
    vs, faces = SF.mesh("sphere66")
    full = SF.case("sphere66", 0.6, "own")
    for cap, V_out, counts in ((0, 66, []), (1, 61, UNIT[:1]), (3, 55, UNIT)):
        c = SF.run("sphere66", full.target, "own", True, cap)
        assert not c.reached and c.vs.shape[0] == V_out and c.counts == counts
        # refused: of the round that was analysed and not applied -- SO.candidates on the mesh the capped run returns
        assert c.refused == SO.candidates(c.vs, c.faces, SO.vertex_quadrics(vs, faces)[c.vertex_ids])[1]
        assert c.counts == full.counts[:cap] and (cap == 0) == (c.vs.tobytes() == vs.tobytes())
    one = SF.run("sphere66", 65, "own")
    legal, _ = SO.candidates(vs, faces, SO.vertex_quadrics(vs, faces))
    top = max(legal, key=lambda e: legal[e][0])
    assert one.counts == [(192, 1, 1)] and one.reached and int(np.setdiff1d(np.arange(66), one.vertex_ids)[0]) == legal[top][2]
    none = SF.run("sphere66", 66, "own")
    assert none.counts == [] and none.reached and none.vs.tobytes() == vs.tobytes() and np.array_equal(none.faces, faces)
    assert np.array_equal(none.vertex_ids, np.arange(66)) and np.array_equal(none.coarse_of, np.arange(66)) and none.refused == 0


def test_torus32x24_rounds():
    c = SF.case("torus32x24", 0.6, "sum")
    assert c.in_faces.shape[0] * 3 == 4608 and c.reached and len(c.counts) == 23 and c.refused == 12
    assert c.counts[:3] == [(2304, 308, 25), (2229, 283, 18), (2175, 265, 14)] and max(w for _, _, w in c.counts) >= 25


def test_big_torus_is_a_closed_manifold_past_the_sorts_switch():
    vs, faces = SF.big_torus()
    V = vs.shape[0]
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    assert (V, faces.shape[0]) == (196608, 393216) and a.shape[0] == 1179648 > 1 << 20
    assert np.unique(a * V + b).shape[0] == a.shape[0] and (cnt == 2).all() and V - und.shape[0] + faces.shape[0] == 0
    assert np.isfinite(vs).all() and np.unique(faces).shape[0] == V
    need = V - int(V * 0.6)
    assert 3 * (faces.shape[0] - 2 * need) < 1 << 20         # the last rounds of ratio 0.6 sort fewer keys than the switch
