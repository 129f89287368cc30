"""numpy restatement of semigcn_amd/remesh.py (its module docstring is the specification): serial, dictionary-based, one
edge and one face at a time -- no sort of packed keys, no scans, no atomics; nothing here is shared with the kernels.

float32 arithmetic is done on numpy float32 scalars one operation at a time (so every intermediate is rounded to float32,
in the specified order), the guard on Python floats (float64) the same way."""
from __future__ import annotations

import numpy as np

MASK = 0xFFFFFFFF


def hash32(x):
    x &= MASK
    x ^= x >> 16
    x = (x * 0x7FEB352D) & MASK
    x ^= x >> 15
    x = (x * 0x846CA68B) & MASK
    x ^= x >> 16
    return x


def split_threshold(target):
    return np.float32((4.0 / 3.0 * float(target)) ** 2)


# ---- the edge table ---------------------------------------------------------------------------------------------------------
def edge_table(faces):
    """{(lo, hi): [half-edges h = 3 f + k in ascending h]} and {(lo, hi): rank in ascending (lo, hi) order}."""
    table = {}
    for f, tri in enumerate(faces):
        for k in range(3):
            a, b = int(tri[k]), int(tri[(k + 1) % 3])
            table.setdefault((min(a, b), max(a, b)), []).append(3 * f + k)
    rank = {e: r for r, e in enumerate(sorted(table))}
    return table, rank


def check_input(vs, faces):
    """Raises ValueError as the module does; returns the counts otherwise (all zero)."""
    vs, faces = np.asarray(vs), np.asarray(faces).reshape(-1, 3)
    degenerate = [f for f, t in enumerate(faces) if len({int(t[0]), int(t[1]), int(t[2])}) < 3]
    nonfinite = [v for v in range(vs.shape[0]) if not np.isfinite(vs[v]).all()]
    table, _ = edge_table(faces)
    nonmanifold = sorted(e for e, hs in table.items() if len(hs) >= 3)
    misoriented = sorted(e for e, hs in table.items() if len(hs) == 2 and
                         faces[hs[0] // 3][hs[0] % 3] == faces[hs[1] // 3][hs[1] % 3])
    counts = dict(n_nonmanifold=len(nonmanifold), n_misoriented=len(misoriented), n_degenerate=len(degenerate),
                  n_nonfinite=len(nonfinite), bad_edge=min(nonmanifold + misoriented, default=(-1, -1)),
                  bad_face=min(degenerate, default=-1), bad_vertex=min(nonfinite, default=-1))
    if nonmanifold or misoriented or degenerate or nonfinite:
        raise ValueError(f"the mesh cannot be refined: {counts}")
    return counts


def len2(vs, lo, hi):
    d = [np.float32(vs[hi][i]) - np.float32(vs[lo][i]) for i in range(3)]
    return np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- 1. split ---------------------------------------------------------------------------------------------------------------
def select_split(vs, faces, thr2):
    """The selected edges of one round in ascending rank, and the number of long edges."""
    table, rank = edge_table(faces)
    prio = {}
    for e in table:
        l2 = len2(vs, *e)
        if l2 > thr2:
            prio[e] = (bits(l2), hash32(rank[e]), -rank[e])
    selected = []
    for e in sorted(prio):
        wins = True
        for h in table[e]:
            tri = faces[h // 3]
            for k in range(3):
                a, b = int(tri[k]), int(tri[(k + 1) % 3])
                other = (min(a, b), max(a, b))
                if other != e and other in prio and prio[other] > prio[e]:
                    wins = False
        if wins:
            selected.append(e)
    return selected, len(prio), table


def split_round(vs, faces, thr2):
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    selected, n_long, table = select_split(vs, faces, thr2)
    V, F = vs.shape[0], faces.shape[0]
    new_vs = [((np.float32(vs[lo]) + np.float32(vs[hi])) * np.float32(0.5)).astype(np.float32) for lo, hi in selected]
    mid = {e: V + s for s, e in enumerate(selected)}
    split_faces = {}                                       # face -> (corner k that starts the edge, new vertex)
    for e in selected:
        for h in table[e]:
            assert h // 3 not in split_faces, "two selected edges in one face"
            split_faces[h // 3] = (h % 3, mid[e])
    out = faces.copy()
    extra = []
    for f in sorted(split_faces):
        k, m = split_faces[f]
        a, b, c = (int(faces[f][(k + i) % 3]) for i in range(3))
        out[f] = (a, m, c)
        extra.append((m, b, c))
    if selected:
        vs = np.concatenate([vs, np.stack(new_vs)]).astype(np.float32)
        out = np.concatenate([out, np.array(extra, np.int64).reshape(-1, 3)])
    return vs, out, [list(e) for e in selected], n_long


def split_long_edges(vs, faces, target, max_rounds=64):
    """(vs, faces, parents, counts, n_long)"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    check_input(vs, faces)
    thr2 = split_threshold(target)
    parents = [[i, i] for i in range(vs.shape[0])]
    counts = []
    rounds = 0
    while True:
        new_vs, new_faces, ends, n_long = split_round(vs, faces, thr2)
        if not ends or rounds >= max_rounds:
            break
        vs, faces = new_vs, new_faces
        parents += ends
        counts.append(len(ends))
        rounds += 1
    return vs, faces, np.array(parents, np.int64).reshape(-1, 2), counts, n_long


# ---- 2. flip ----------------------------------------------------------------------------------------------------------------
def valences(faces):
    """({v: number of distinct edges}, set of border vertices)"""
    table, _ = edge_table(faces)
    val, border = {}, set()
    for (lo, hi), hs in table.items():
        val[lo] = val.get(lo, 0) + 1
        val[hi] = val.get(hi, 0) + 1
        if len(hs) == 1:
            border.update((lo, hi))
    return val, border


def deviation(faces):
    val, border = valences(faces)
    return sum(abs(n - (4 if v in border else 6)) for v, n in val.items())


def _normal(vs, p, q, r):
    u = [float(vs[q][i]) - float(vs[p][i]) for i in range(3)]
    v = [float(vs[r][i]) - float(vs[p][i]) for i in range(3)]
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def guard(vs, a, b, c, d):
    old = (_normal(vs, a, b, c), _normal(vs, b, a, d))
    new = (_normal(vs, a, d, c), _normal(vs, d, b, c))
    return all(_dot(n, o) > 0.0 for n in new for o in old)


def flip_candidates(vs, faces):
    """{edge: (priority, (a, b, c, d), (f0, f1))} of one round."""
    table, rank = edge_table(faces)
    val, border = valences(faces)
    tgt = lambda v: 4 if v in border else 6
    cands = {}
    for e, hs in table.items():
        if len(hs) != 2:
            continue
        h0, h1 = hs
        f0, k0, f1, k1 = h0 // 3, h0 % 3, h1 // 3, h1 % 3
        a, b, c = (int(faces[f0][(k0 + i) % 3]) for i in range(3))
        d = int(faces[f1][(k1 + 2) % 3])
        if c == d or (min(c, d), max(c, d)) in table:
            continue
        if val[a] - 1 < (2 if a in border else 3) or val[b] - 1 < (2 if b in border else 3):
            continue
        before = sum(abs(val[v] - tgt(v)) for v in (a, b, c, d))
        after = sum(abs(val[v] - 1 - tgt(v)) for v in (a, b)) + sum(abs(val[v] + 1 - tgt(v)) for v in (c, d))
        gain = before - after
        if gain <= 0 or not guard(vs, a, b, c, d):
            continue
        cands[e] = ((gain, hash32(rank[e]), -rank[e]), (a, b, c, d), (f0, f1))
    return cands


def flip_round(vs, faces):
    """(faces, the selected edges with their quads)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cands = flip_candidates(vs, faces)
    at = {}
    for e, (p, quad, _) in cands.items():
        for v in quad:
            at.setdefault(v, []).append(e)
    selected = []
    for e in sorted(cands):
        p, quad, _ = cands[e]
        if all(cands[o][0] <= p for v in quad for o in at[v]):
            selected.append(e)
    out = faces.copy()
    for e in selected:
        _, (a, b, c, d), (f0, f1) = cands[e]
        out[f0] = (a, d, c)
        out[f1] = (d, b, c)
    return out, [(e, cands[e][1]) for e in selected]


def flip_edges(vs, faces, max_rounds=32):
    """(faces, flips per round, deviation before, deviation after, the deviation after every round)"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    check_input(vs, faces)
    before = deviation(faces)
    flips, trail = [], [before]
    while len(flips) < max_rounds:
        new_faces, selected = flip_round(vs, faces)
        if not selected:
            break
        faces = new_faces
        flips.append(len(selected))
        trail.append(deviation(faces))
    return faces, flips, before, trail[-1], trail


# ---- 3. / 4. relax, project, the pipeline (float64 smoothing and a brute-force closest point: for CPU checks of fixtures) ------
def border_vertices(faces, V):
    flags = np.zeros(V, bool)
    flags[list(valences(faces)[1])] = True
    return flags


def closest_points(pts, svs, sfaces):
    from mesh_distance_oracle import point_triangles
    A, B, C = (np.asarray(svs, np.float64)[np.asarray(sfaces)[:, k]] for k in range(3))
    out = np.zeros((len(pts), 3))
    dist = np.zeros(len(pts))
    for i, p in enumerate(np.asarray(pts, np.float64)):
        d, c, _, _ = point_triangles(p, A, B, C)
        k = int(np.argmin(d))
        out[i], dist[i] = c[k], d[k]
    return out, dist


def relax_project(vs, faces, svs, sfaces, steps=1):
    import prepare_oracle as PO
    vs = np.asarray(vs, np.float32)
    interior = ~border_vertices(faces, vs.shape[0])
    moved = PO.smooth(vs, faces, steps, movable=interior).astype(np.float32)
    closest = closest_points(moved, svs, sfaces)[0].astype(np.float32)
    return np.where(interior[:, None], closest, vs).astype(np.float32)


def refine_mesh(vs, faces, target, iterations=5, relax_steps=1):
    """(vs, faces, parents) -- positions agree with the device only to rounding (float64 here, float32 there)."""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    svs, sfaces = vs.copy(), faces.copy()
    parents = np.repeat(np.arange(vs.shape[0])[:, None], 2, 1)
    for _ in range(iterations):
        vs, faces, par, _, _ = split_long_edges(vs, faces, target)
        parents = np.concatenate([parents, par[parents.shape[0]:]])
        faces = flip_edges(vs, faces)[0]
        vs = relax_project(vs, faces, svs, sfaces, relax_steps)
    return vs, faces, parents


# ---- invariants ---------------------------------------------------------------------------------------------------------------
def euler(faces, V=None):
    table, _ = edge_table(faces)
    used = {int(v) for v in np.asarray(faces).reshape(-1)}
    return len(used) - len(table) + len(faces)


def directed_once(faces):
    seen = set()
    for tri in np.asarray(faces):
        for k in range(3):
            e = (int(tri[k]), int(tri[(k + 1) % 3]))
            if e in seen:
                return False
            seen.add(e)
    return True


def max_len2(vs, faces):
    vs = np.asarray(vs, np.float32)
    return max(len2(vs, *e) for e in edge_table(faces)[0])


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def one_triangle():
    """Edges of length 3, 4, 5 (len2 9, 16, 25)."""
    return np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def two_triangles():
    """The shared edge {0, 2} (len2 32) is the longest."""
    return (np.array([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int64))


def fan8(pulled=False):
    """A hub (vertex 0, valence 8) inside a convex octagon with integer coordinates (vertices 1 .. 8, all on the border).
    Every spoke is a flip candidate of gain 2, and all of them share the hub.  ``pulled``: rim vertex 1 moves from (2, 1) to
    (1, 0.5), inside the chord from vertex 8 to vertex 2: the quad (0, 8, 1, 2) is concave at vertex 1 and the guard
    refuses to replace its diagonal {0, 1} by {8, 2}."""
    rim = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)]
    vs = np.array([(0, 0, 0)] + [(x, y, 0) for x, y in rim], np.float32)
    if pulled:
        vs[1] = (1, 0.5, 0)
    faces = np.array([(0, 1 + i, 1 + (i + 1) % 8) for i in range(8)], np.int64)
    return vs, faces


def tetrahedron():
    vs = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64)
    return vs, faces


def grid(n=8, step=1.0):
    """Open n x n-quad grid with integer coordinates, diagonal (i, j) -> (i + 1, j + 1)."""
    idx = lambda i, j: i * (n + 1) + j
    vs = np.array([[i * step, j * step, 0] for i in range(n + 1) for j in range(n + 1)], np.float32)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return vs, np.array(faces, np.int64)


def stretched_torus(nu, nv, stretch=3.0, **kw):
    from semigcn_amd import synth
    m = synth.torus_mesh(nu, nv, masks=False, **kw)
    vs = (m.vs * np.array([stretch, 1.0, 1.0])).astype(np.float32)
    return vs, m.faces.astype(np.int64)


def median_edge(vs, faces):
    return float(np.median([np.sqrt(float(len2(vs, *e))) for e in edge_table(faces)[0]]))
