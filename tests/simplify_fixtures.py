"""Fixtures of the simplify stage, shared by tests/test_simplify_oracle.py (their premises, on the CPU) and
tests/test_gpu_simplify.py and tests/test_gpu_simplify_edges.py (the device).  Everything here is numpy and the serial
oracle (tests/simplify_oracle.py); nothing is shared with the kernels.  ``case(name, ratio, quadrics)`` runs the oracle once
per process and hands out read-only arrays; ``run`` is the same with a vertex budget and a round cap."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import remesh_open_fixtures as OF
import remesh_oracle as RO
import simplify_oracle as SO


def sphere(level=3):
    from semigcn_amd import synth
    m = synth.octahedron_sphere(level)
    return m.vs.astype(np.float32), m.faces.astype(np.int64)


def torus20x12():
    from semigcn_amd import synth
    m = synth.torus_mesh(20, 12, masks=False)
    return m.vs.astype(np.float32), m.faces.astype(np.int64)


def valence3():
    """The 18-vertex sphere with face 0 split in three by a vertex (18, valence 3) at its centroid, pushed out to the sphere."""
    vs, faces = sphere(1)
    a, b, c = (int(v) for v in faces[0])
    p = vs[[a, b, c]].astype(np.float64).mean(0)
    vs = np.concatenate([vs, (p / np.linalg.norm(p)).astype(np.float32)[None]])
    faces = np.concatenate([[[a, b, 18]], faces[1:], [[b, c, 18], [c, a, 18]]]).astype(np.int64)
    return vs, faces


def foldover():
    """``RO.grid(4, 4.0)`` (flat, integer coordinates: every cost is exactly 0) with the interior vertices moved by integers
    in [-2, 2] in the plane, seed 18: no input face is reversed, the edge of highest priority is {5, 11}, and moving 11 onto
    the border vertex 5 reverses a face."""
    vs, faces = RO.grid(4, 4.0)
    interior = [i for i in range(25) if 0 < i // 5 < 4 and 0 < i % 5 < 4]
    vs = vs.copy()
    vs[interior, :2] += np.random.default_rng(18).integers(-2, 3, (len(interior), 2)).astype(np.float32)
    return vs, faces


def foldover_mid():
    """``RO.grid(5, 4.0)`` with the interior vertices moved as in ``foldover``, seed 23: no input face is reversed, the edge of
    highest priority is {19, 26}, both ends interior, and moving 19 to the midpoint of the edge reverses a face."""
    vs, faces = RO.grid(5, 4.0)
    interior = [i for i in range(36) if 0 < i // 6 < 5 and 0 < i % 6 < 5]
    vs = vs.copy()
    vs[interior, :2] += np.random.default_rng(23).integers(-2, 3, (len(interior), 2)).astype(np.float32)
    return vs, faces


def flat_grid():
    """``RO.grid(5)`` lifted to z = 2: flat, integer coordinates, every quadric entry an integer."""
    vs, faces = RO.grid(5)
    vs = vs.copy()
    vs[:, 2] = 2.0
    return vs, faces


FIXTURES = {"sphere258": sphere, "torus20x12": torus20x12, "wavy12": OF.wavy12, "holed20x12": OF.holed20x12,
            "tetrahedron": RO.tetrahedron, "valence3": valence3, "foldover": foldover, "foldover_mid": foldover_mid,
            "flat_grid": flat_grid, "sphere66": lambda: sphere(2)}
OPEN = ("wavy12", "holed20x12", "foldover", "foldover_mid", "flat_grid")
#: what the device is compared on: (fixture, ratio)
CASES = [("sphere258", 0.6), ("sphere258", 0.2), ("torus20x12", 0.6), ("wavy12", 0.6), ("holed20x12", 0.6), ("foldover", 0.6),
         ("foldover_mid", 0.6), ("valence3", 0.6), ("flat_grid", 0.6), ("sphere66", 0.6)]


# ---- the edge fixtures: clauses of the rule that no fixture above executes (tests/test_gpu_simplify_edges.py) -----------------
# "Oracle:" in a docstring is the time of ``SO.simplify`` for one (fixture, budget, quadrics) on one CPU core; on a busy
# machine it has been 1.5 times that.
def _glue(vs_a, faces_a, vs_b, faces_b, shared_a, shared_b):
    """Two meshes that share ONE vertex: ``shared_b`` of the second is translated onto ``shared_a`` of the first (a float32
    subtraction and addition per coordinate) and takes its id; the other vertices of the second follow the first's, in order."""
    shift = vs_a[shared_a] - vs_b[shared_b]
    vs_b = (vs_b + shift).astype(np.float32)
    new = np.empty(vs_b.shape[0], np.int64)
    others = np.arange(vs_b.shape[0]) != shared_b
    new[others] = vs_a.shape[0] + np.arange(vs_b.shape[0] - 1)
    new[shared_b] = shared_a
    return np.concatenate([vs_a, vs_b[others]]).astype(np.float32), np.concatenate([faces_a, new[faces_b]]).astype(np.int64)


def _sheet(n, seed):
    """``RO.grid(n)`` with heights in {0, 1/4, 1/2, 3/4} (seeded), 0 at vertex 0: a sheet that is not flat, so its costs are not
    all 0, with coordinates that are exact in every format."""
    vs, faces = RO.grid(n)
    vs = vs.copy()
    vs[:, 2] = np.random.default_rng(seed).integers(0, 4, vs.shape[0]).astype(np.float32) * np.float32(0.25)
    vs[0, 2] = 0.0
    return vs, faces


#: the vertex the two parts of a touching fixture share
TOUCH = 0


def touch_closed():
    """Two 66-vertex spheres that touch in vertex 0: the second is the first mirrored in x with its faces reversed (still
    outward) and moved so that its vertex 0 lands on the first's.  V = 131, F = 256; vertex 0 has valence 8 and two closed
    fans of 4 faces.  Oracle: 0.4 s at ratio 0.6."""
    vs, faces = sphere(2)
    return _glue(vs, faces, vs * np.array([-1, 1, 1], np.float32), faces[:, ::-1], TOUCH, TOUCH)


def touch_open():
    """Two 4 x 4 sheets (``_sheet``) that share the border corner 0, the second turned into the plane y = 0 on the far side
    (x, z <= 0): at vertex 0 two open fans of 2 faces touch, ``val`` is 3 + 3, and the two diagonals (0, 6) and (0, 30) are
    its only eligible edges.  V = 49.  Oracle: 0.05 s at ratio 0.7 (0.6 cannot be reached: 31 of the 49 are border
    vertices)."""
    vs_a, faces_a = _sheet(4, 11)
    vs_b, faces_b = _sheet(4, 12)
    vs_b = np.stack([-vs_b[:, 0], vs_b[:, 2], -vs_b[:, 1]], 1)
    return _glue(vs_a, faces_a, vs_b, faces_b, TOUCH, TOUCH)


def touch_mixed():
    """The 66-vertex sphere whose vertex 0 -- (r, 0, 0) -- is also the border corner 0 of a 3 x 3 sheet (``_sheet``) that
    leaves it towards +x: a closed fan of 4 faces and an open fan of 2.  The four sphere edges at vertex 0 are eligible (one
    border end) and keep vertex 0.  V = 81.  Oracle: 0.2 s at ratio 0.6."""
    vs, faces = sphere(2)
    vs_b, faces_b = _sheet(3, 13)
    return _glue(vs, faces, vs_b, faces_b, TOUCH, TOUCH)


#: the vertex of ``flat_face`` that is moved onto the edge across it, and the face that becomes flat
FLAT_V = 14
FLAT_FACE = (14, 7, 13)


def flat_face():
    """``RO.grid(5)`` with heights ``default_rng(5).integers(0, 4) * 0.25`` and vertex 14 moved to the float32 midpoint
    ``(vs[x] + vs[y]) * 0.5f`` of the edge across it in its face ``(14, x, y) = `` ``FLAT_FACE``: three distinct, collinear
    corners, ``nn == 0`` exactly.  Oracle: 0.05 s at ratio 0.6."""
    vs, faces = RO.grid(5)
    vs = vs.copy()
    vs[:, 2] = np.random.default_rng(5).integers(0, 4, vs.shape[0]).astype(np.float32) * np.float32(0.25)
    x, y = FLAT_FACE[1:]
    vs[FLAT_V] = (vs[x] + vs[y]) * np.float32(0.5)
    return vs, faces


#: sphere66 times float32(2**k)
SCALES = (60, 100, -70, -80, -140)


def scaled(k):
    """The 66-vertex sphere times ``float32(2**k)``: an exact scaling while nothing is subnormal.  Oracle: 0.3 s (9 or 10
    rounds) or 0.5 s (17 rounds) at ratio 0.6."""
    def make():
        vs, faces = sphere(2)
        return vs * np.float32(2.0 ** k), faces
    return make


HUB_N = 80


def hub_sphere():
    """Two poles of valence 80 and two rings of 80 vertices at latitudes +-30 degrees, radius 3: V = 162, F = 320.  Ids: north
    pole 0, the northern ring 1..80, the southern ring 81..160 (half a step on), south pole 161: the north pole is the kept end
    of its 80 edges, the south pole the removed end of its 80.  Every footprint holds a pole.  Oracle: 4.6 s at ratio 0.6 (50
    rounds of one or two winners)."""
    n = HUB_N
    t = 2.0 * np.pi * np.arange(n) / n
    c = np.sqrt(0.75)
    ring = lambda z, off: np.stack([c * np.cos(t + off), c * np.sin(t + off), np.full(n, z)], 1)
    vs = np.concatenate([[[0, 0, 1]], ring(0.5, 0.0), ring(-0.5, np.pi / n), [[0, 0, -1]]]) * 3.0
    i = np.arange(n)
    j = (i + 1) % n
    up, lo = 1 + i, 1 + n + i
    faces = np.concatenate([np.stack([np.zeros(n, np.int64), up, 1 + j], 1), np.stack([up, lo, 1 + j], 1),
                            np.stack([1 + j, lo, 1 + n + j], 1), np.stack([np.full(n, 2 * n + 1), 1 + n + j, lo], 1)])
    return vs.astype(np.float32), faces.astype(np.int64)


DISC_N = 80
#: the centre of ``hub_disc``
DISC_CENTRE = DISC_N
DISC_RATIO = 0.8


def hub_disc():
    """A flat open disc in the plane z = 2: a border ring of 80 vertices (0..79) at radius 2, the centre (vertex 80, valence
    80) and a ring of 80 interior vertices (81..160) at radius 1, half a step behind the border ring.  Every cost is exactly 0
    (``flat_grid``), so the hash alone orders and the centre's edges win like any other.  The numbering puts the centre's
    edges at ranks 240..319 of the 400, and rank 315 has the largest hash of all: the first round's best edge is (80, 156),
    which keeps the centre.  V = 161, F = 240.  Oracle: 1.6 s at ratio 0.8."""
    n = DISC_N
    t = 2.0 * np.pi * np.arange(n) / n
    ring = lambda r, off: np.stack([r * np.cos(t + off), r * np.sin(t + off), np.full(n, 2.0)], 1)
    vs = np.concatenate([ring(2.0, np.pi / n), [[0, 0, 2.0]], ring(1.0, 0.0)])
    i = np.arange(n)
    j = (i + 1) % n
    a, b = n + 1 + i, i
    faces = np.concatenate([np.stack([np.full(n, n), a, n + 1 + j], 1), np.stack([a, b, n + 1 + j], 1),
                            np.stack([n + 1 + j, b, j], 1)])
    return vs.astype(np.float32), faces.astype(np.int64)


#: the ids of the vertices of ``unused3`` that no face uses
UNUSED = (0, 30, 68)


def unused3():
    """The 66-vertex sphere with three vertices no face uses, at ids 0, 30 and 68, somewhere finite.  V = 69.  Oracle: 0.5 s at
    ratio 0.6 (0.2 s), 0.3 s down to ``target_v = 5`` (which stops at 7)."""
    vs, faces = sphere(2)
    used = np.setdiff1d(np.arange(69), UNUSED)
    out = np.empty((69, 3), np.float32)
    out[used] = vs
    out[list(UNUSED)] = np.array([[7.5, -2.25, 1e3], [0.0, 0.0, 0.0], [-1e-3, 4.0, 0.125]], np.float32)
    return out, used[faces]


def torus32x24():
    """``synth.torus_mesh(32, 24, masks=False)``: 768 vertices, 4608 half-edges, 18 workgroups.  Oracle: 5.3 s at ratio
    0.6 with "sum" (23 rounds)."""
    from semigcn_amd import synth
    m = synth.torus_mesh(32, 24, masks=False)
    return m.vs.astype(np.float32), m.faces.astype(np.int64)


def big_torus(nu=512, nv=384, seed=7):
    """A closed nu x nv torus grid (diagonal (u, v) -> (u + 1, v + 1)) with every vertex moved by N(0, 0.05), built with
    vectorised numpy: at 512 x 384, V = 196 608, F = 393 216 and 3 F = 1 179 648 half-edges, above the 1 048 576 at which
    rocPRIM's radix sort goes from a merge sort to onesweep.  No oracle is run on it."""
    u, v = (x.ravel() for x in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))
    up, vp = (u + 1) % nu, (v + 1) % nv
    a, b, c, d = u * nv + v, up * nv + v, up * nv + vp, u * nv + vp
    faces = np.empty((2 * nu * nv, 3), np.int64)
    faces[0::2] = np.stack([a, b, c], 1)
    faces[1::2] = np.stack([a, c, d], 1)
    th, ph = 2 * np.pi * u / nu, 2 * np.pi * v / nv
    R, r = nu / (2 * np.pi), nv / (4 * np.pi)
    vs = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], 1)
    vs = vs + np.random.default_rng(seed).normal(0.0, 0.05, vs.shape)
    return vs.astype(np.float32), faces


FIXTURES.update({"touch_closed": touch_closed, "touch_open": touch_open, "touch_mixed": touch_mixed, "flat_face": flat_face,
                 "hub_sphere": hub_sphere, "hub_disc": hub_disc, "unused3": unused3, "torus32x24": torus32x24})
FIXTURES.update({f"sphere66_2^{k}": scaled(k) for k in SCALES})
#: what tests/test_gpu_simplify_edges.py compares bit for bit: (fixture, ratio, the values of ``quadrics``)
EDGE_CASES = [("touch_closed", 0.6, ("own", "sum")), ("touch_open", 0.7, ("own", "sum")), ("touch_mixed", 0.6, ("own", "sum")),
              ("flat_face", 0.6, ("own", "sum"))] + [(f"sphere66_2^{k}", 0.6, ("own", "sum")) for k in SCALES] + [
              ("hub_sphere", 0.6, ("own", "sum")), ("hub_disc", DISC_RATIO, ("own", "sum")), ("unused3", 0.6, ("own", "sum")),
              ("torus32x24", 0.6, ("sum",))]


@functools.lru_cache(maxsize=None)
def mesh(name):
    vs, faces = FIXTURES[name]()
    vs, faces = np.ascontiguousarray(vs, np.float32), np.ascontiguousarray(faces, np.int64)
    vs.setflags(write=False)
    faces.setflags(write=False)
    return vs, faces


def case(name, ratio, quadrics="own", guard=True):
    return run(name, int(mesh(name)[0].shape[0] * ratio), quadrics, guard)


@functools.lru_cache(maxsize=None)
def run(name, target, quadrics="own", guard=True, max_rounds=256):
    """The oracle on ``mesh(name)`` down to ``target`` vertices, once per process."""
    vs, faces = mesh(name)
    out = SO.simplify(vs, faces, target, quadrics=quadrics, max_rounds=max_rounds, guard=guard)
    for a in out[:4]:
        a.setflags(write=False)
    return SimpleNamespace(name=name, in_vs=vs, in_faces=faces, target=target, vs=out[0], faces=out[1], vertex_ids=out[2],
                           coarse_of=out[3], counts=out[4], reached=out[5], refused=out[6])


def trace(name, target, quadrics="own", max_rounds=256):
    """The oracle's loop (``SO.simplify``) round by round: yields (vs, faces, legal, winners, val) of every round that collapses
    something -- the mesh the round starts with, ``SO.candidates`` on it, the winning edges and ``RO.valences``."""
    vs, faces = mesh(name)
    Q = SO.vertex_quadrics(vs, faces)
    n = 0
    while vs.shape[0] > target and faces.shape[0] > 0:
        legal, _ = SO.candidates(vs, faces, Q)
        out = SO.simplify_round(vs, faces, Q, vs.shape[0] - target, quadrics)
        if out[5][2] == 0 or n >= max_rounds:
            break
        gone = set(np.setdiff1d(np.arange(vs.shape[0]), out[3]).tolist())
        winners = [e for e in legal if legal[e][2] in gone and out[4][legal[e][2]] == out[4][legal[e][1]]]
        assert len(winners) == out[5][2]
        yield vs, faces, legal, winners, RO.valences(faces)[0]
        vs, faces, Q = out[0], out[1], out[2]
        n += 1


def fans(faces, v):
    """The sizes (in faces) of the fans at ``v``, descending: the classes of the faces at ``v`` under sharing an edge at ``v``."""
    at = [t for t in faces.tolist() if v in t]
    group = list(range(len(at)))
    for i, s in enumerate(at):
        for j, t in enumerate(at):
            if len(set(s) & set(t)) == 2:
                gi, gj = group[i], group[j]
                group = [gi if g == gj else g for g in group]
    return sorted((group.count(g) for g in set(group)), reverse=True)


def edge_counts(faces):
    """{(lo, hi): number of faces}"""
    return {e: len(hs) for e, hs in RO.edge_table(faces)[0].items()}


def euler(vs, faces):
    return vs.shape[0] - len(edge_counts(faces)) + faces.shape[0]
