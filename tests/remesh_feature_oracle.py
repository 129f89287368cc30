"""numpy restatement of the "Creases" section of semigcn_amd/remesh.py (its module docstring is the specification), and the
fixtures of tests/test_remesh_feature_fixtures.py (their premises, on the CPU) and tests/test_gpu_remesh_features.py (the
device).  Serial and dictionary-based like tests/remesh_oracle.py and tests/collapse_oracle.py, whose candidate functions it
wraps (``creased``); nothing here is shared with the kernels.

The predicate and the straightness guard run on Python floats (float64) one operation at a time, the crease step on numpy
float32 scalars.  The umbrella smoothing and the two closest-point queries of relax_project are *primitives* here: by default
the float64 restatements (``prepare_oracle.smooth``, a brute-force closest point), which agree with the device to rounding;
the GPU test hands in the device's own ``laplacian_smooth`` and ``Surface.query`` -- each pinned by its own tests -- so that
what this file restates (the classes, who moves, the crease step, what is projected where, the topology) compares bit for bit."""
from __future__ import annotations

import contextlib
import functools
import math

import numpy as np

import collapse_oracle as CO
import remesh_oracle as RO

SMOOTH, LINE, CORNER, BORDER = 0, 1, 2, 3
CLOSING_PASSES = 4


def feature_cos(angle_deg):
    return float(np.cos(np.radians(np.float64(angle_deg))))


# ---- 1. the predicate and the classes ------------------------------------------------------------------------------------
def is_crease(vs, a, b, c, d, cos_t):
    """(a, b, c) is the face of the lower half-edge, (b, a, d) the other one."""
    n1, n2 = RO._normal(vs, a, b, c), RO._normal(vs, b, a, d)
    dd = RO._dot(n1, n2)
    q = RO._dot(n1, n1) * RO._dot(n2, n2)
    c2 = cos_t * cos_t
    if cos_t >= 0:
        return dd < 0 or dd * dd < c2 * q
    return dd < 0 and dd * dd > c2 * q


def _quad(faces, hs):
    h0, h1 = hs
    f0, k0, f1, k1 = h0 // 3, h0 % 3, h1 // 3, h1 % 3
    a, b, c = (int(faces[f0][(k0 + i) % 3]) for i in range(3))
    return a, b, c, int(faces[f1][(k1 + 2) % 3])


def crease_set(vs, faces, cos_t):
    """The crease edges (lo, hi) of the mesh as a set; empty when ``cos_t`` is None."""
    if cos_t is None:
        return set()
    table, _ = RO.edge_table(faces)
    creases = {e for e, hs in table.items() if len(hs) == 2 and is_crease(vs, *_quad(faces, hs), cos_t)}
    if SEEN is not None:
        SEEN.append(len(creases))
    return creases


#: a list that receives the number of crease edges of every evaluation (every round of every stage), or None
SEEN = None


def crease_counts(creases):
    """({v: nc}, {v: sorted crease neighbours})"""
    nbrs = {}
    for lo, hi in creases:
        nbrs.setdefault(lo, []).append(hi)
        nbrs.setdefault(hi, []).append(lo)
    return {v: len(n) for v, n in nbrs.items()}, {v: sorted(n) for v, n in nbrs.items()}


def features(vs, faces, cos_t):
    """(vclass uint8 [V], crease_nbr int64 [V, 2], crease edges int64 [C, 2] in ascending (lo, hi))"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    V = vs.shape[0]
    creases = crease_set(vs, faces, cos_t)
    nc, nbrs = crease_counts(creases)
    border = RO.valences(faces)[1]
    vclass = np.zeros(V, np.uint8)
    nbr = np.full((V, 2), -1, np.int64)
    for v in range(V):
        if v in border:
            vclass[v] = BORDER
        elif nc.get(v, 0) == 2:
            vclass[v] = LINE
            nbr[v] = (min(nbrs[v]), max(nbrs[v]))
        elif nc.get(v, 0) != 0:
            vclass[v] = CORNER
    return vclass, nbr, np.array(sorted(creases), np.int64).reshape(-1, 2)


# ---- 2. flip and collapse: the candidate functions of the two oracles, wrapped ----------------------------------------------
def flip_candidates(vs, faces, cos_t, _base=RO.flip_candidates):
    creases = crease_set(vs, faces, cos_t)
    return {e: c for e, c in _base(vs, faces).items() if e not in creases}


def kept_vertex(a, b, border, nc):
    """The kept end of the edge {a, b} (not both on a border), in the order of precedence of the specification."""
    if a in border or b in border:
        return a if a in border else b
    na, nb = nc.get(a, 0), nc.get(b, 0)
    if (na > 0) != (nb > 0):
        return a if na > 0 else b
    if na > 0 and (na != 2) != (nb != 2):
        return a if na != 2 else b
    return min(a, b)


def _plain_candidate(vs, faces, table, val, border, at, hs, k, r, thr2):
    """The conditions of 2a. for a given choice of k and r, as tests/collapse_oracle.py states them: the ring of r when all
    hold, None otherwise."""
    h0, h1 = hs
    c = int(faces[h0 // 3][(h0 % 3 + 2) % 3])
    d = int(faces[h1 // 3][(h1 % 3 + 2) % 3])
    floor = lambda v: 2 if v in border else 3
    if c == d:
        return None
    fan = CO._fan(faces, at, r, k)
    if fan is None:
        return None
    ring = [x for _, x, _ in fan]
    others = [w for w in ring if w != k]
    if len([w for w in others if CO._edge(k, w) in table]) != 2:
        return None
    if val[c] - 1 < floor(c) or val[d] - 1 < floor(d) or val[k] + val[r] - 4 < floor(k):
        return None
    if any(CO.len2(vs, *CO._edge(k, w)) > thr2 for w in others):
        return None
    if not all(CO._dot(CO._normal(vs, r, x, y), CO._normal(vs, k, x, y)) > 0.0 for _, x, y in fan if k not in (x, y)):
        return None
    return ring


def straight(vs, k, r, w):
    """u . v > 0 with u = p_r - p_k and v = p_w - p_r, float64 differences of the float32 coordinates."""
    u = [float(vs[r][i]) - float(vs[k][i]) for i in range(3)]
    v = [float(vs[w][i]) - float(vs[r][i]) for i in range(3)]
    return RO._dot(u, v) > 0.0


def collapse_candidates(vs, faces, lo2, thr2, cos_t, log=None, _base=CO.collapse_candidates):
    """{edge: (priority, k, r, footprint)} of one round with the crease rules.  An edge without a crease at either end is
    taken from ``CO.collapse_candidates`` as it stands; for every other short edge the conditions of 2a. are evaluated for
    the kept vertex the creases choose (and checked against the plain oracle where that is the same vertex).  ``log``: a
    list that receives, per short two-face edge with a removable end, (edge, k, r, plain conditions hold, refusal) with
    refusal one of None, "corner", "off-crease", "bent"."""
    plain = _base(vs, faces, lo2, thr2)
    creases = crease_set(vs, faces, cos_t)
    nc, nbrs = crease_counts(creases)
    table, rank = RO.edge_table(faces)
    val, border = RO.valences(faces)
    at = {}
    for f, tri in enumerate(faces):
        for v in tri:
            at.setdefault(int(v), []).append(f)
    cands = {}
    for e, hs in table.items():
        l2 = RO.len2(vs, *e)
        a, b = e
        if len(hs) != 2 or not l2 < lo2 or (a in border and b in border):
            continue
        k = kept_vertex(a, b, border, nc)
        r = b if k == a else a
        if nc.get(a, 0) == 0 and nc.get(b, 0) == 0:
            ring = list(plain[e][3] - {r}) if e in plain else None
            assert e not in plain or plain[e][1:3] == (k, r)
        else:
            ring = _plain_candidate(vs, faces, table, val, border, at, hs, k, r, thr2)
            plain_k = a if a in border else (b if b in border else min(a, b))
            assert plain_k != k or (ring is not None) == (e in plain)
        refusal = None
        if nc.get(r, 0) not in (0, 2):
            refusal = "corner"
        elif nc.get(r, 0) == 2 and e not in creases:
            refusal = "off-crease"
        elif nc.get(r, 0) == 2:
            other, = [w for w in nbrs[r] if w != k]
            if not straight(vs, k, r, other):
                refusal = "bent"
        if log is not None:
            log.append((e, k, r, ring is not None, refusal))
        if ring is None or refusal is not None:
            continue
        cands[e] = ((RO.MASK - RO.bits(l2), RO.hash32(rank[e]), -rank[e]), k, r, frozenset([r] + ring))
    return cands


@contextlib.contextmanager
def creased(cos_t, log=None):
    """``RO.flip_round`` / ``RO.flip_edges`` and ``CO.select_collapse`` / ``CO.collapse_short_edges`` with the crease rules
    while the block runs (``cos_t`` None: unchanged)."""
    keep = (RO.flip_candidates, CO.collapse_candidates)
    if cos_t is not None:
        RO.flip_candidates = lambda vs, faces, _b=keep[0]: flip_candidates(vs, faces, cos_t, _b)
        CO.collapse_candidates = lambda vs, faces, lo2, thr2, _b=keep[1]: collapse_candidates(vs, faces, lo2, thr2, cos_t, log, _b)
    try:
        yield
    finally:
        RO.flip_candidates, CO.collapse_candidates = keep


def flip_edges(vs, faces, cos_t, max_rounds=32):
    with creased(cos_t):
        return RO.flip_edges(vs, faces, max_rounds)


def collapse_short_edges(vs, faces, target, cos_t, max_rounds=128):
    with creased(cos_t):
        return CO.collapse_short_edges(vs, faces, target, max_rounds)


# ---- 3. relax and project ---------------------------------------------------------------------------------------------------
def crease_step(R, nbr):
    """One Jacobi step: (R[v] + R[lo] + R[hi]) / 3 per component in float32, summed in that order."""
    R = np.asarray(R, np.float32)
    out = R.copy()
    three = np.float32(3.0)
    for v in np.flatnonzero(nbr[:, 0] >= 0):
        lo, hi = int(nbr[v, 0]), int(nbr[v, 1])
        for i in range(3):
            out[v, i] = np.float32(np.float32(np.float32(R[v, i] + R[lo, i]) + R[hi, i]) / three)
    return out


def smooth_f64(vs, faces, steps, movable):
    import prepare_oracle as PO
    return PO.smooth(vs, faces, steps, movable=movable).astype(np.float32)


def closest_f64(pts, svs, sfaces):
    return RO.closest_points(pts, svs, sfaces)[0].astype(np.float32)


def closest_on_segments_f64(pts, svs, edges):
    """Brute force, float64: the closest point of the segments ``edges`` into ``svs`` to every point."""
    svs, out = np.asarray(svs, np.float64), []
    A, B = svs[np.asarray(edges)[:, 0]], svs[np.asarray(edges)[:, 1]]
    D = B - A
    den = (D * D).sum(1)
    for p in np.asarray(pts, np.float64):
        t = np.clip(((p - A) * D).sum(1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        c = A + t[:, None] * D
        out.append(c[int(np.argmin(((c - p) ** 2).sum(1)))])
    return np.array(out, np.float64).reshape(-1, 3).astype(np.float32)


PRIMITIVES = dict(smooth=smooth_f64, closest=closest_f64, closest_seg=closest_on_segments_f64)


def project_by_class(P, moved_smooth, moved_line, vclass, svs, sfaces, seg_edges, prim):
    out = np.asarray(P, np.float32).copy()
    s, l = vclass == SMOOTH, vclass == LINE
    if s.any():
        out[s] = prim["closest"](moved_smooth[s], svs, sfaces)
    if l.any() and len(seg_edges):
        out[l] = prim["closest_seg"](moved_line[l], svs, seg_edges)
    return out


def relax_project(vs, faces, svs, sfaces, seg_edges, cos_t, steps=1, **prim):
    """``seg_edges``: the crease edges of the surface ``(svs, sfaces)``, [C, 2] (empty: crease-line vertices stay)."""
    prim = {**PRIMITIVES, **prim}
    P = np.asarray(vs, np.float32)
    vclass, nbr, _ = features(P, faces, cos_t)
    Q = prim["smooth"](P, faces, steps, vclass == SMOOTH) if steps > 0 else P
    R = P
    for _ in range(steps):
        R = crease_step(R, nbr)
    return project_by_class(P, np.asarray(Q, np.float32), R, vclass, svs, sfaces, seg_edges, prim)


def refine_mesh(vs, faces, target, cos_t, iterations=5, relax_steps=1, collapse=False, **prim):
    """(vs, faces, report): the pipeline of ``remesh.refine_mesh`` with the crease rules, closing passes included.  The
    report holds the counts the device reports."""
    prim = {**PRIMITIVES, **prim}
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    svs, sfaces = vs.copy(), faces.copy()
    vclass, _, seg = features(vs, faces, cos_t)
    report = {"n_crease_edges_start": len(seg), "n_corners_start": int((vclass == CORNER).sum()), "iterations": [], "closing": []}
    for _ in range(iterations):
        vs, faces, _, counts, n_long = RO.split_long_edges(vs, faces, target)
        entry = {"split": counts, "n_long": n_long}
        if collapse:
            vs, faces, _, _, entry["collapse"], entry["n_short_after_collapse"] = collapse_short_edges(vs, faces, target, cos_t)
        faces, entry["flip"], entry["deviation_after_split"], entry["deviation_after_flip"], _ = flip_edges(vs, faces, cos_t)
        vs = relax_project(vs, faces, svs, sfaces, seg, cos_t, relax_steps, **prim)
        report["iterations"].append(entry)
    for _ in range(CLOSING_PASSES + 1 if iterations > 0 else 1):
        last = len(report["closing"]) == CLOSING_PASSES or iterations == 0
        n_before = vs.shape[0]
        vs, faces, _, counts, n_long = RO.split_long_edges(vs, faces, target, max_rounds=0 if last else 64)
        if not counts:
            break
        report["closing"].append(sum(counts))
        vclass = features(vs, faces, cos_t)[0].copy()
        vclass[:n_before] = BORDER                                 # only the inserted vertices are projected
        vs = project_by_class(vs, vs, vs, vclass, svs, sfaces, seg, prim)
    vclass, _, edges = features(vs, faces, cos_t)
    report.update({"n_long": n_long, "n_crease_edges_end": len(edges), "n_corners_end": int((vclass == CORNER).sum()),
                   "n_short": CO.n_short(vs, faces, CO.collapse_threshold(target)), "deviation_end": RO.deviation(faces)})
    return vs, faces, report


# ---- measures ---------------------------------------------------------------------------------------------------------------
def volume(vs, faces):
    """The signed tetrahedron sum in float64."""
    p = np.asarray(vs, np.float64)
    a, b, c = (p[np.asarray(faces)[:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


def distance_to_segments(pts, svs, edges):
    """float64 distance of every point to the closest of the segments."""
    pts = np.asarray(pts, np.float64)
    if len(pts) == 0:
        return np.zeros(0)
    svs = np.asarray(svs, np.float64)
    A, B = svs[np.asarray(edges)[:, 0]], svs[np.asarray(edges)[:, 1]]
    D = B - A
    den = (D * D).sum(1)
    out = []
    for p in pts:
        t = np.clip(((p - A) * D).sum(1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        out.append(np.sqrt((((A + t[:, None] * D) - p) ** 2).sum(1).min()))
    return np.array(out)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def cube():
    """The unit cube, vertex 4 x + 2 y + z, outward normals: 12 creases of 90 degrees, 8 corners with nc = 3; the six face
    diagonals are flat."""
    vs = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    faces = np.array([(0, 1, 3), (0, 3, 2), (4, 7, 5), (4, 6, 7), (0, 5, 1), (0, 4, 5), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                      (1, 7, 3), (1, 5, 7)], np.int64)
    return vs, faces


def hinge60():
    """The tetrahedron a = (0, 0, 0), b = (1, -1, -1), c = (0, 0, -1), d = (1, -2, -1) with the faces (a, b, c), (b, a, d),
    (c, b, d), (a, c, d).  Across {a, b}: n1 = (1, 1, 0), n2 = (1, 0, 1), dd = 1, q = 4 -- 60 degrees, an exact tie at cos_t = 0.5."""
    vs = np.array([(0, 0, 0), (1, -1, -1), (0, 0, -1), (1, -2, -1)], np.float32)
    return vs, np.array([(0, 1, 2), (1, 0, 3), (2, 1, 3), (0, 2, 3)], np.int64)


def roof(n=4):
    """An open strip of 2 x n quads bent by 90 degrees along the ridge y = 0: vertex (x, y, -|y|), index 3 x + (y + 1).  The ridge
    vertices 1 .. n - 1 are crease-line; the ridge ends and everything else lie on the border."""
    vs = np.array([(x, y, -abs(y)) for x in range(n + 1) for y in (-1, 0, 1)], np.float32)
    idx = lambda x, y: 3 * x + (y + 1)
    faces = []
    for x in range(n):
        for y in (-1, 0):
            a, b, c, d = idx(x, y), idx(x + 1, y), idx(x + 1, y + 1), idx(x, y + 1)
            faces += [(a, b, c), (a, c, d)]
    return vs, np.array(faces, np.int64)


def _prism(poly, zs, cap, centre=None):
    """A closed prism over the counter-clockwise polygon ``poly`` with one vertex ring per entry of ``zs``; ``cap``: the
    polygon's triangles (counter-clockwise index triples; the index len(poly) names ``centre``, a vertex of its own per cap)."""
    m, nz = len(poly), len(zs)
    vs = [(x, y, z) for z in zs for x, y in poly]
    faces = []
    for r in range(nz - 1):
        for i in range(m):
            j = (i + 1) % m
            a, b, c, d = r * m + i, r * m + j, (r + 1) * m + j, (r + 1) * m + i
            faces += [(a, b, c), (a, c, d)]
    lo_c = hi_c = None
    if centre is not None:
        lo_c, hi_c = len(vs), len(vs) + 1
        vs += [(centre[0], centre[1], zs[0]), (centre[0], centre[1], zs[-1])]
    for i, j, k in cap:
        low = [lo_c if t == m else t for t in (i, j, k)]
        high = [hi_c if t == m else (nz - 1) * m + t for t in (i, j, k)]
        faces += [(low[0], low[2], low[1]), tuple(high)]
    return np.array(vs, np.float32), np.array(faces, np.int64)


def prism16(rings=3, radius=2.0):
    """A 16-gon prism with ``rings`` vertex rings and fan caps: the two rims are closed creases of 90 degrees whose polylines
    turn by 22.5 degrees per vertex; the side faces turn by 22.5 degrees, below 30; the middle rings and the cap centres are
    smooth.  At radius 2 a rim edge is 0.78 long: at the fixture's target 0.6 neither long nor short, so the rims keep their 16
    corners and the sides stay below the angle (a rim that a collapse coarsens to 45 degrees per vertex turns the sides into
    creases: the rule allows that)."""
    poly = [(radius * math.cos(2 * math.pi * i / 16), radius * math.sin(2 * math.pi * i / 16)) for i in range(16)]
    return _prism(poly, list(range(rings)), [(16, i, (i + 1) % 16) for i in range(16)], centre=(0.0, 0.0))


def l_prism():
    """An L-shaped prism of height 1: convex creases and the reflex one at (1, 1); all 12 vertices are corners with nc = 3."""
    poly = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    return _prism(poly, [0, 1], [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)])


def pyramid():
    """A closed square pyramid, base corners (+-1, +-1, 0) = vertices 0 .. 3, apex (0, 0, 1) = vertex 4.  At 30 degrees the apex
    is a corner with nc = 4 and the base corners have nc = 3; at 120 degrees only the base edges (135 degrees) are creases."""
    vs = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), (0, 0, 1)], np.float32)
    faces = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (0, 2, 1), (0, 3, 2)], np.int64)
    return vs, faces


BENT_HUB, BENT_TARGET = 0, 10.0


def bent():
    """A plateau corner: vertex 0 = (0, 0, 1) with the plateau z = 1 over x <= 0 <= y (vertices 1 = (-1, 0, 1), 2 = (0, 1, 1),
    3 = (-1, 1, 1)), slopes of 45 degrees down to z = 0 outside, and a cone fan of four faces (22.5 degrees each) round the
    corner.  The plateau's rim 1 - 0 - 2 is the only crease at vertex 0 and turns by exactly 90 degrees there: u . v = 0.  Open;
    every vertex but 0 is on the border.  At ``BENT_TARGET`` every edge is short and no length guard holds."""
    fan = [(math.cos(math.radians(t)), math.sin(math.radians(t)), 0.0) for t in (-90.0, -67.5, -45.0, -22.5, 0.0)]
    fan[0], fan[4] = (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)
    vs = [(0, 0, 1), (-1, 0, 1), (0, 1, 1), (-1, 1, 1), (-1, -1, 0)] + fan + [(1, 1, 0)]     # 4: eave a, 5 .. 9: fan, 10: eave b
    faces = [(0, 2, 3), (0, 3, 1), (1, 4, 5), (1, 5, 0)] + [(0, 5 + i, 6 + i) for i in range(4)] + [(0, 9, 10), (0, 10, 2)]
    return np.array(vs, np.float32), np.array(faces, np.int64)


#: the smooth control is refined to this multiple of its median edge
SMOOTH_TARGET = 0.8


def smooth_control():
    """A regular torus fine enough that no edge is a crease at 30 degrees in any round of one iteration with collapse
    (tests/test_remesh_feature_fixtures.py asserts it)."""
    return RO.stretched_torus(32, 24, stretch=1.0, flip_frac=0.0, jitter=0.0)


FIXTURES = {"cube": cube, "hinge60": hinge60, "roof": roof, "prism16": prism16, "l_prism": l_prism, "pyramid": pyramid, "bent": bent}
#: name -> the target the fixture is refined to
TARGETS = {"cube": 0.25, "hinge60": 0.6, "roof": 0.5, "prism16": 0.6, "l_prism": 0.4, "pyramid": 0.5, "bent": 0.5}
COS30 = feature_cos(30.0)
