"""Brute-force numpy restatement of semigcn_amd.repair: the predicate of its module docstring evaluated on every pair of
faces whose boxes touch (an O(F^2) box prefilter, chunked; no hierarchy, no stack, no two passes, no sort), the repair loop
composed from this oracle, tests/components_oracle.py, tests/holes_oracle.py and tests/prepare_oracle.py, and the meshes the
tests share.

Integer input (an integer dtype) is evaluated in int64: for |coordinates| <= 2^10 every determinant is below 2^37 and
exact.  Float input is read as the float32 values the device sees and evaluated in float64, in the order of operations the
specification writes down.  On float input a pair is *marginal* when any determinant evaluated for it has a magnitude below
1e-9 x the product of the norms of its difference vectors (three for orient3d, two for orient2d): the sign of such a
determinant is not to be trusted, and a test input must have none."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import components_oracle as CO
import holes_oracle as HO

MARGIN = 1e-9


@dataclass
class Result:
    pairs: np.ndarray          # int64 [P, 2], i < j, sorted lexicographically
    face_mask: np.ndarray      # bool [F]
    n_degenerate: int
    marginal: np.ndarray       # int64 [M, 2]: candidate pairs with a determinant too small to trust (float input only)

    def __len__(self):
        return self.pairs.shape[0]


class _Eval:
    """Signs of determinants over arrays of candidate pairs; remembers which pairs saw a marginal one."""

    def __init__(self, n, exact):
        self.exact = exact
        self.marginal = np.zeros(n, bool)

    def _note(self, det, vecs, active):
        if self.exact:
            return
        scale = np.ones(det.shape[0])
        for v in vecs:
            scale = scale * np.sqrt((v.astype(np.float64) ** 2).sum(-1))
        self.marginal |= active & (np.abs(det) < MARGIN * scale)

    def o3(self, a, b, c, d, active):
        u, v, w = a - d, b - d, c - d
        det = (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])
               + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]))
        self._note(det, (u, v, w), active)
        return np.sign(det).astype(np.int64)

    def o2(self, a, b, c, active):
        u, v = a - c, b - c
        det = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        self._note(det, (u, v), active)
        return np.sign(det).astype(np.int64)


def _proj(p, axis):
    return np.stack([np.where(axis == 0, p[:, 1], p[:, 0]), np.where(axis == 2, p[:, 1], p[:, 2])], 1)


def _same_side(s1, s2, s3):
    return ((s1 >= 0) & (s2 >= 0) & (s3 >= 0)) | ((s1 <= 0) & (s2 <= 0) & (s3 <= 0))


def _seg_seg(ev, p, q, c, d, active):
    s1, s2, s3, s4 = ev.o2(p, q, c, active), ev.o2(p, q, d, active), ev.o2(c, d, p, active), ev.o2(c, d, q, active)
    collinear = (s1 == 0) & (s2 == 0) & (s3 == 0) & (s4 == 0)
    lo = np.maximum(np.minimum(p, q), np.minimum(c, d))
    hi = np.minimum(np.maximum(p, q), np.maximum(c, d))
    return np.where(collinear, (lo <= hi).all(1), (s1 * s2 <= 0) & (s3 * s4 <= 0))


def _seg_tri(ev, p, q, a, b, c, axis, active):
    """closed segment pq against the closed triangle abc, row by row"""
    sp, sq = ev.o3(a, b, c, p, active), ev.o3(a, b, c, q, active)
    off = active & ((sp != 0) | (sq != 0))
    cross = off & (sp * sq <= 0)
    s1, s2, s3 = ev.o3(p, q, a, b, cross), ev.o3(p, q, b, c, cross), ev.o3(p, q, c, a, cross)
    hit = cross & _same_side(s1, s2, s3)
    flat = active & ~off
    if flat.any():
        P, Q, A, B, C = (_proj(x, axis) for x in (p, q, a, b, c))
        inside = np.zeros_like(flat)
        for X in (P, Q):
            inside |= _same_side(ev.o2(A, B, X, flat), ev.o2(B, C, X, flat), ev.o2(C, A, X, flat))
        for (c0, c1) in ((A, B), (B, C), (C, A)):
            inside |= _seg_seg(ev, P, Q, c0, c1, flat)
        hit |= flat & inside
    return hit


def _normals(X, faces):
    a, b, c = X[faces[:, 0]], X[faces[:, 1]], X[faces[:, 2]]
    e1, e2 = b - a, c - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def _candidates(X, faces, ok, chunk=256):
    """(i, j), i < j, of the faces whose closed boxes meet, in lexicographic order"""
    P = X[faces]
    lo, hi = P.min(1), P.max(1)
    F = faces.shape[0]
    out = []
    for s in range(0, F, chunk):
        e = min(s + chunk, F)
        meet = ((lo[s:e, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[s:e, None, :])).all(2)
        meet &= np.arange(F)[None, :] > np.arange(s, e)[:, None]
        meet &= ok[s:e, None] & ok[None, :]
        i, j = np.nonzero(meet)
        out.append(np.stack([i + s, j], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def self_intersections(vs, faces) -> Result:
    vs = np.asarray(vs)
    exact = np.issubdtype(vs.dtype, np.integer)
    X = vs.astype(np.int64) if exact else vs.astype(np.float32).astype(np.float64)
    X = X.reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    if F == 0:
        return Result(np.zeros((0, 2), np.int64), np.zeros(0, bool), 0, np.zeros((0, 2), np.int64))
    n = _normals(X, f)
    degenerate = CO.degenerate(f) | (n == 0).all(1)
    axis = np.argmax(np.abs(n), 1)                         # the first of equals: the lowest axis
    cand = _candidates(X, f, ~degenerate)
    fi, fj = f[cand[:, 0]], f[cand[:, 1]]
    ai, aj = axis[cand[:, 0]], axis[cand[:, 1]]
    N = cand.shape[0]
    ev = _Eval(N, exact)
    rows = np.arange(N)
    match = fi[:, :, None] == fj[:, None, :]               # [N, 3 (slot in i), 3 (slot in j)]
    in_i, in_j = match.any(2), match.any(1)
    shared = in_i.sum(1)
    Ti = [X[fi[:, k]] for k in range(3)]
    Tj = [X[fj[:, k]] for k in range(3)]
    hit = shared == 3

    none = shared == 0
    for e in range(3):
        hit |= _seg_tri(ev, Ti[e], Ti[(e + 1) % 3], Tj[0], Tj[1], Tj[2], aj, none)
        hit |= _seg_tri(ev, Tj[e], Tj[(e + 1) % 3], Ti[0], Ti[1], Ti[2], ai, none)

    one = shared == 1
    if one.any():
        k, kh = np.argmax(in_i, 1), np.argmax(in_j, 1)
        hit |= _seg_tri(ev, X[fi[rows, (k + 1) % 3]], X[fi[rows, (k + 2) % 3]], Tj[0], Tj[1], Tj[2], aj, one)
        hit |= _seg_tri(ev, X[fj[rows, (kh + 1) % 3]], X[fj[rows, (kh + 2) % 3]], Ti[0], Ti[1], Ti[2], ai, one)

    two = shared == 2
    if two.any():
        k, kb = np.argmin(in_i, 1), np.argmin(in_j, 1)
        a, u, v, b = X[fi[rows, k]], X[fi[rows, (k + 1) % 3]], X[fi[rows, (k + 2) % 3]], X[fj[rows, kb]]
        flat = two & (ev.o3(u, v, a, b, two) == 0)
        U, V = _proj(u, ai), _proj(v, ai)
        hit |= flat & (ev.o2(U, V, _proj(a, ai), flat) * ev.o2(U, V, _proj(b, ai), flat) > 0)

    pairs = cand[hit]
    mask = np.zeros(F, bool)
    mask[pairs.reshape(-1)] = True
    return Result(pairs, mask, int(degenerate.sum()), cand[ev.marginal])


# ---- the repair loop -----------------------------------------------------------------------------------------------------
def _fill(vs, faces, max_hole_edges, fair_steps):
    import prepare_oracle as PO
    out_vs, out_faces, inserted, _filled, _loops = HO.fill_holes(vs, faces, max_hole_edges)
    if fair_steps > 0 and inserted.any():
        out_vs = PO.smooth(out_vs, out_faces, fair_steps, movable=inserted)
    return out_vs.astype(np.float32), out_faces, inserted


def repair_oracle(vs, faces, grow=1, max_rounds=10, max_hole_edges=None, fair_steps=30, whole_stage=True):
    """(vs float32, faces, rounds, removed_per_round, remaining, vertex_ids): semigcn_amd.repair.repair (whole_stage) or
    remove_self_intersections, with float64 fairing rounded to float32 after every fill."""
    vs = np.asarray(vs, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.arange(vs.shape[0], dtype=np.int64)

    def fill(vs, faces, ids):
        vs, faces, inserted = _fill(vs, faces, max_hole_edges, fair_steps)
        return vs, faces, np.concatenate([ids, np.full(vs.shape[0] - ids.shape[0], -1, np.int64)])

    if whole_stage:
        vs, faces, vid, _fid, _kept = CO.keep_components(vs, faces, "largest")
        ids = ids[vid]
        if faces.shape[0]:
            vs, faces, ids = fill(vs, faces, ids)
    rounds, removed = 0, []
    while True:
        hits = self_intersections(vs, faces)
        if len(hits) == 0 or rounds >= max_rounds:
            return vs, faces, rounds, removed, len(hits), ids
        drop = hits.face_mask
        for _ in range(grow):
            touched = np.zeros(vs.shape[0], bool)
            touched[faces[drop].reshape(-1)] = True
            drop = touched[faces].any(1)
        removed.append(int(drop.sum()))
        vs, faces, vid, _fid, _kept = CO.keep_components(vs, faces[~drop], "largest")
        ids = ids[vid]
        if faces.shape[0]:
            vs, faces, ids = fill(vs, faces, ids)
        rounds += 1


# ---- meshes ------------------------------------------------------------------------------------------------------------
def hand_cases():
    """name -> (vs int64 [V, 3], faces, the pairs by hand, n_degenerate by hand); one per branch of the predicate."""
    T = [[0, 0, 0], [8, 0, 0], [0, 8, 0]]                   # the triangle most cases are tested against, in z = 0
    c = {}
    # the edge (2,2,-3)-(2,2,3) of face 1 goes through the interior of face 0
    c["edge_pierces_interior"] = (T + [[2, 2, -3], [2, 2, 3], [9, 9, 3]], [[0, 1, 2], [3, 4, 5]], [(0, 1)], 0)
    # face 1 stands on face 0: its vertex (2,2,0) lies exactly on it, the rest is above
    c["endpoint_on_face_touches"] = (T + [[2, 2, 0], [2, 3, 4], [3, 2, 4]], [[0, 1, 2], [3, 4, 5]], [(0, 1)], 0)
    # coplanar, face 1 strictly inside face 0: no edge of either crosses the other in space
    c["coplanar_one_inside"] = (T + [[1, 1, 0], [3, 1, 0], [1, 3, 0]], [[0, 1, 2], [3, 4, 5]], [(0, 1)], 0)
    c["coplanar_disjoint"] = (T + [[9, 9, 0], [12, 9, 0], [9, 12, 0]], [[0, 1, 2], [3, 4, 5]], [], 0)
    # two faces that meet in vertex 0 only
    c["shared_vertex_clean"] = (T + [[-8, 0, 2], [0, -8, 2]], [[0, 1, 2], [0, 3, 4]], [], 0)
    # face 1 = (vertex 0, (4,4,-4), (2,2,4)): its edge opposite vertex 0 goes through (3,3,0), inside face 0
    c["shared_vertex_opposite_edge_pierces"] = (T + [[4, 4, -4], [2, 2, 4]], [[0, 1, 2], [0, 3, 4]], [(0, 1)], 0)
    # both on the edge 0-1, both apexes on the same side of it in z = 0: folded flat
    c["shared_edge_folded_flat"] = (T + [[4, 3, 0]], [[0, 1, 2], [1, 0, 3]], [(0, 1)], 0)
    # the same with the second apex lifted by one unit: the fold is open
    c["shared_edge_fold_opened"] = (T + [[4, 3, 1]], [[0, 1, 2], [1, 0, 3]], [], 0)
    c["duplicate_faces"] = (T, [[0, 1, 2], [2, 0, 1]], [(0, 1)], 0)
    # face 1 repeats vertex 3, face 2 has collinear vertices: both lie across face 0 and still are in no pair
    c["degenerate_faces"] = (T + [[2, 2, -3], [2, 2, 3], [2, 2, 0], [2, 2, 6]], [[0, 1, 2], [3, 3, 4], [3, 5, 6]], [], 2)
    return {k: (np.asarray(v, np.int64), np.asarray(f, np.int64), np.asarray(p, np.int64).reshape(-1, 2), d)
            for k, (v, f, p, d) in c.items()}


def flat_grid(n=8, step=1):
    """n x n quads in z = 0, two faces each, integer coordinates: everything coplanar, nothing overlaps."""
    x, y = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    vs = np.stack([x.ravel() * step, y.ravel() * step, np.zeros((n + 1) ** 2, np.int64)], 1).astype(np.int64)
    a = (x[:-1, :-1] * (n + 1) + y[:-1, :-1]).ravel()
    b, d = a + (n + 1), a + 1
    c = b + 1
    return vs, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)


def box(n, size, origin):
    """The surface of a cube of edge ``size`` at ``origin``, n x n quads per side, welded, integer coordinates."""
    step = size // n
    assert step * n == size
    index, vs, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(vs)
            vs.append([origin[k] + step * p[k] for k in range(3)])
        return index[p]

    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, i + di, j + dj
                        return vid(tuple(p))
                    a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    faces += [[a, b, c], [a, c, d]]
    return np.asarray(vs, np.int64), np.asarray(faces, np.int64)


def two_boxes():
    """Two interpenetrating cubes, 192 + 108 faces less the last one: F = 299 is no multiple of 4 (a partial leaf) or of
    64 (a partial wavefront, five workgroups).  The second cube's corner edges meet the first one's sides on the
    diagonals of their quads: exact zeros."""
    v0, f0 = box(4, 8, (0, 0, 0))
    v1, f1 = box(3, 9, (3, 3, 3))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + v0.shape[0]])[:-1]


def crossed_grid(n=30, big_first=True):
    """An n x n grid with integer heights 0, 2, 4 and one large triangle lying slightly tilted at height 2 to 3 across all
    of it: that face has hundreds of partners.  ``big_first``: the large triangle is face 0 (every pair is found from it:
    one face counts and emits hundreds of rows, and every other face's offset lies behind them); otherwise it is the last
    face (hundreds of faces add to one face's count)."""
    vs, faces = flat_grid(n)
    vs = vs * np.array([2, 2, 0]) + np.stack([np.zeros(len(vs), np.int64)] * 2 + [2 * ((7 * vs[:, 0] + 3 * vs[:, 1]) % 3)], 1)
    big = np.array([[-80, -80, 2], [200, -80, 2], [-80, 200, 3]], np.int64)
    V = vs.shape[0]
    tri = np.array([[V, V + 1, V + 2]], np.int64)
    return np.concatenate([vs, big]), np.concatenate([tri, faces] if big_first else [faces, tri])


def torus_pair(nu=40, nv=38, seed=314):
    """Two jittered tori (synth.torus_mesh, seeds ``seed`` and ``seed + 1``) pushed into each other: float32."""
    from semigcn_amd import synth
    a, b = synth.torus_mesh(nu, nv, seed=seed, masks=False), synth.torus_mesh(nu, nv, seed=seed + 1, masks=False)
    R, r = max(nu / (2 * np.pi), 2.0 * nv / (2 * np.pi)), nv / (2 * np.pi)
    vb = b.vs + np.array([0.7 * R, 0.0, 0.3 * r])
    return (np.concatenate([a.vs, vb]).astype(np.float32), np.concatenate([a.faces, b.faces + a.vs.shape[0]]))


def scaled_integers(mesh, scale=512):
    """(vs int64, faces) of a synth mesh with its coordinates multiplied by ``scale`` and rounded (|coordinates| stay below
    2^12: the determinants are below 2^42, still exact in float64)."""
    return np.rint(np.asarray(mesh.vs, np.float64) * scale).astype(np.int64), np.asarray(mesh.faces, np.int64)


def folded_sphere(level=4, cap=0.5, depth=2.3, axis=(0.3, 0.5, 0.81)):
    """synth.octahedron_sphere(level) with the cap around ``axis`` pushed through the opposite side: the vertices whose
    height h along the axis exceeds (1 - cap) radius move against it by ``depth`` radius x sin^2 of their way from the
    cap's rim to its pole.  The axis is a generic direction, so that the fold does not inherit the octahedron's
    symmetries (coplanar and mirror-image pairs).  One component, watertight, self-intersecting.  float32."""
    from semigcn_amd import synth
    m = synth.octahedron_sphere(level)
    vs = np.array(m.vs, np.float64)
    d = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    rad = np.linalg.norm(vs, axis=1).mean()
    t = np.clip((vs @ d / rad - (1.0 - cap)) / cap, 0.0, 1.0)          # 0 at the rim and below, 1 at the pole
    vs -= (depth * rad * np.sin(0.5 * np.pi * t) ** 2)[:, None] * d[None, :]
    return vs.astype(np.float32), np.asarray(m.faces, np.int64)


# ---- degenerate soups: every slot, axis and winding of the predicate -------------------------------------------------------
SPACING = 32                # between cluster centres; a cluster's coordinates stay within +-12 of its centre

FLATNESS = ("generic", "z in {0, 1}", "z = 0", "z = x + y", "z = x")


def signed_axis_permutations():
    """The 48 maps x -> sign * x[perm] of the cube onto itself, as (perm, sign) pairs of int64 [3]."""
    import itertools
    return [(np.array(p, np.int64), np.array(s, np.int64)) for p in itertools.permutations(range(3))
            for s in itertools.product((1, -1), repeat=3)]


def cluster_centres(n, spacing=SPACING):
    """int64 [n, 3]: the first n points of a cubic grid of that spacing, centred on the origin."""
    side = 1
    while side ** 3 < n:
        side += 1
    g = np.stack(np.unravel_index(np.arange(n), (side, side, side)), 1).astype(np.int64)
    return (2 * g - (side - 1)) * (spacing // 2)


def _assemble(clusters, spacing=SPACING):
    """[(vs, faces)] of integer clusters -> one mesh, cluster c moved to the c-th grid centre; also the first face of each."""
    centres = cluster_centres(len(clusters), spacing)
    vs, faces, first, nv, nf = [], [], [], 0, 0
    for (v, f), c in zip(clusters, centres):
        assert np.abs(v).max() <= 12
        vs.append(v + c)
        faces.append(f + nv)
        first.append(nf)
        nv += v.shape[0]
        nf += f.shape[0]
    vs = np.concatenate(vs).astype(np.int64)
    assert np.abs(vs).max() <= 2 ** 10
    return vs, np.concatenate(faces).astype(np.int64), np.asarray(first + [nf], np.int64)


def soup_cluster(c, rng, R=3, n_vertices=7, n_faces=12):
    """Cluster c of soup_clusters about the origin: (vs int64 [7, 3], faces int64 [12, 3])."""
    v = rng.integers(-R, R + 1, (n_vertices, 3))
    kind = c % len(FLATNESS)
    if kind == 1:
        v[:, 2] = rng.integers(0, 2, n_vertices)
    elif kind == 2:
        v[:, 2] = 0
    elif kind == 3:
        v[:, 2] = v[:, 0] + v[:, 1]                          # normal (1, 1, -1): all three axes tie
    elif kind == 4:
        v[:, 2] = v[:, 0]                                   # normal (1, 0, -1): two axes tie
    f = np.stack([rng.choice(n_vertices, 3, replace=(c % 8 == 7)) for _ in range(n_faces)])
    perm, sign = signed_axis_permutations()[c % 48]
    v = v[:, perm] * sign
    if c % 2:
        f = f[:, ::-1]
    return v.astype(np.int64), np.ascontiguousarray(f).astype(np.int64)


def soup_clusters(n=125, seed=2024, R=3, n_vertices=7, n_faces=12):
    """n random triangle soups of 7 integer vertices in [-R, R]^3 and 12 faces each, on a grid of spacing 32 so that the
    boxes of two clusters cannot touch: (vs int64, faces int64); cluster c owns vertices 7 c .. 7 c + 6 and faces
    12 c .. 12 c + 11.  Faces draw 3 of the 7 ids without repetition, in every eighth cluster with (repeated ids).  The
    flatness cycles through FLATNESS; cluster c is then mapped through the (c mod 48)-th signed axis permutation and
    every second cluster has the winding of its faces reversed.  |coordinates| <= 2^10.  Seed 2024 is the first one
    tried; tests/test_intersect_exact.py asserts what it has to provide."""
    rng = np.random.default_rng(seed)
    vs, faces, _ = _assemble([soup_cluster(c, rng, R, n_vertices, n_faces) for c in range(n)])
    return vs, faces


ORBIT_MAPS = (((2, 0, 1), (1, 1, 1)),         # (x, y, z) -> (z, x, y): the plane z = 0 becomes x = 0
              ((1, 2, 0), (-1, 1, 1)),        # (x, y, z) -> (-y, z, x): z = 0 becomes y = 0
              ((1, 0, 2), (1, 1, 1)))         # (x, y, z) -> (y, x, z): z = 0 stays, mirrored


def hand_case_orbit():
    """Every hand case in every labelling: (vs int64, faces, pairs int64 [P, 2], n_degenerate), the pairs and the count
    by hand (relabelled), not from any oracle.  Two-face cases: the 6 vertex orders of face 0 x the 6 of face 1 x both
    face orders; degenerate_faces: its 6 face orders x 6 vertex orders (face m takes order p + m).  The whole set three
    times, under ORBIT_MAPS.  Each variant is a cluster of its own on the grid of soup_clusters."""
    import itertools
    orders = list(itertools.permutations(range(3)))
    clusters, pairs, n_deg, nf = [], [], 0, 0
    for perm, sign in ORBIT_MAPS:
        for name, (v, f, want, d) in hand_cases().items():
            v = v[:, list(perm)] * np.array(sign)
            if f.shape[0] == 2:
                variants = [((a, b), fo) for a in range(6) for b in range(6) for fo in ((0, 1), (1, 0))]
            else:
                variants = [(tuple((p + m) % 6 for m in range(3)), fo) for p in range(6)
                            for fo in itertools.permutations(range(3))]
            for vo, fo in variants:
                g = np.stack([f[m][list(orders[vo[m]])] for m in range(f.shape[0])])[list(fo)]   # new face k = old fo[k]
                new_of_old = np.argsort(fo)
                for i, j in want.tolist():
                    pairs.append(sorted((nf + int(new_of_old[i]), nf + int(new_of_old[j]))))
                clusters.append((v, g))
                n_deg += d
                nf += g.shape[0]
    vs, faces, _ = _assemble(clusters)
    pairs = np.asarray(sorted(pairs), np.int64).reshape(-1, 2)
    return vs, faces, pairs, n_deg


def dyadic(vs, offset=(3.5, -1.25, 0.75)):
    """Integer coordinates x 2^-7 plus a dyadic offset, float32: not integers, and every determinant still exact."""
    out = np.asarray(vs, np.float64) * 2.0 ** -7 + np.asarray(offset, np.float64)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def shifted_to_limit(vs, sign):
    """Integer vs translated so that on every axis the largest (sign = +1) or smallest (-1) coordinate is +-1024: the
    documented edge of the exactness claim."""
    vs = np.asarray(vs, np.int64)
    out = vs + (1024 - vs.max(0) if sign > 0 else -1024 - vs.min(0))
    assert np.abs(out).max() == 1024
    return out


def rotated_soups(n=96, seed=2024):
    """The soups of soup_clusters(n, seed) through a fixed rotation (0.6 rad about z, then 1.1 rad about x) x 1/3 plus
    (2.25, -1.5, 3.125), rounded to float32: what was an exact zero determinant is rounding noise now."""
    vs, faces = soup_clusters(n, seed)
    a, b = 0.6, 1.1
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    out = vs.astype(np.float64) @ (Rx @ Rz).T / 3.0 + np.array([2.25, -1.5, 3.125])
    return out.astype(np.float32), faces


def coincident_stack(K=70):
    """K copies of one triangle, each with three vertex rows of its own: nothing is shared by id, every Morton code is
    equal, every leaf box is the same, and all K (K - 1) / 2 pairs cross (face 0 has K - 1 partners above it)."""
    tri = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 3]], np.int64)
    return np.tile(tri, (K, 1)), np.arange(3 * K, dtype=np.int64).reshape(K, 3)


def ladder(big_first, steps=21):
    """Triangles (s, s, s), (1.25 s, s, s), (s, 1.25 s, s) with s = 2^-k, k = 0 .. steps - 1, and one triangle (0, 0, 0),
    (1.25, 0.75, 1), (0.75, 1.25, 1) whose median is the diagonal they all start on, as the first or the last face.
    The centroids halve at every step, so the Morton tree degenerates towards a chain.  float32, all dyadic."""
    vs, faces = [], []
    for k in range(steps):
        s = 2.0 ** -k
        vs += [[s, s, s], [1.25 * s, s, s], [s, 1.25 * s, s]]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    big = [[0.0, 0.0, 0.0], [1.25, 0.75, 1.0], [0.75, 1.25, 1.0]]
    if big_first:
        vs, faces = big + vs, [[0, 1, 2]] + [[i + 3 for i in f] for f in faces]
    else:
        faces.append([3 * steps, 3 * steps + 1, 3 * steps + 2])
        vs += big
    out = np.asarray(vs, np.float64)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32), np.asarray(faces, np.int64)
