"""Fixtures for the remesh stage on OPEN meshes and at ties, shared by tests/test_gpu_remesh_open.py (the device) and
tests/test_remesh_open_fixtures.py (their premises, on the CPU).  Everything here is numpy and the serial oracles
(tests/remesh_oracle.py, tests/collapse_oracle.py); nothing is shared with the kernels.

* ``wavy12`` and ``holed20x12``: a curved, jittered open patch and a torus with two holes, target 0.6 x the median edge.
  ``open_case(name)`` holds the oracle's split, the flip of the split mesh round by round, the collapse of the split mesh and
  the flip after it, each computed once.
* ``altered(...)``: the oracles with one rule changed -- other border flags, a guard that lets a zero dot product pass
  (``>=`` for ``>``), a fused ``len2``.  The CPU tests use them to show that a device with that mistake would give another
  answer on these fixtures, i.e. that the exact comparisons on the device can see it.
* the guard ties: three fans with small integer or half-integer coordinates whose decisive dot product is exactly 0.
* the threshold ties: soups of small components, one edge of each within one ulp of a threshold, found by a seeded search."""
from __future__ import annotations

import contextlib
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import collapse_oracle as CO
import remesh_oracle as RO


# ---- the open meshes ----------------------------------------------------------------------------------------------------
def wavy12():
    """``RO.grid(12)`` lifted to z = 0.8 sin(0.9 x) cos(0.7 y), jittered by N(0, 0.12) per coordinate, x scaled by 3."""
    vs, faces = RO.grid(12)
    vs = vs.astype(np.float64)
    vs[:, 2] = 0.8 * np.sin(0.9 * vs[:, 0]) * np.cos(0.7 * vs[:, 1])
    vs = vs + np.random.default_rng(5).normal(0.0, 0.12, vs.shape)
    return (vs * np.array([3.0, 1.0, 1.0])).astype(np.float32), faces


def holed20x12():
    """The stretched 20 x 12 torus without the faces at the vertices within index distance 2 of (u, v) = (5, 3) and within 1
    of (14, 8); unused vertices dropped."""
    nu, nv = 20, 12
    vs, faces = RO.stretched_torus(nu, nv)
    u, v = np.divmod(np.arange(nu * nv), nv)
    cyc = lambda d, n: np.minimum(d % n, (-d) % n)
    gone = np.zeros(nu * nv, bool)
    for (cu, cv), reach in (((5, 3), 2), ((14, 8), 1)):
        gone |= np.maximum(cyc(u - cu, nu), cyc(v - cv, nv)) <= reach
    faces = faces[~gone[faces].any(1)]
    used = np.unique(faces)
    new = np.full(nu * nv, -1, np.int64)
    new[used] = np.arange(used.shape[0])
    return vs[used], new[faces]


OPEN = {"wavy12": wavy12, "holed20x12": holed20x12}


def numpy_border(faces, V):
    """The ends of the edges with one face."""
    return RO.border_vertices(faces, V)


def flip_trail(vs, faces, max_rounds=32):
    """[faces after 0, 1, 2, ... rounds of ``RO.flip_round``], until a round selects nothing."""
    trail = [np.asarray(faces, np.int64)]
    while len(trail) <= max_rounds:
        new_faces, selected = RO.flip_round(vs, trail[-1])
        if not selected:
            break
        trail.append(new_faces)
    return trail


@functools.lru_cache(maxsize=None)
def open_case(name):
    """vs, faces, target; ``split`` = RO.split_long_edges; ``flip`` = RO.flip_edges of the split mesh and ``flip_faces`` its
    faces after every round; ``collapse`` = CO.collapse_short_edges of the split mesh; ``flip2`` = RO.flip_edges after it."""
    vs, faces = OPEN[name]()
    target = 0.6 * RO.median_edge(vs, faces)
    split = RO.split_long_edges(vs, faces, target)
    flip = RO.flip_edges(split[0], split[1])
    trail = flip_trail(split[0], split[1])
    assert len(trail) == len(flip[1]) + 1 and np.array_equal(trail[-1], flip[0])
    collapse = CO.collapse_short_edges(split[0], split[1], target)
    flip2 = RO.flip_edges(collapse[0], collapse[1])
    for a in (vs, faces) + tuple(x for x in split[:3] + (flip[0],) + collapse[:4] + (flip2[0],)) + tuple(trail):
        a.setflags(write=False)
    return SimpleNamespace(name=name, vs=vs, faces=faces, target=target, split=split, flip=flip, flip_faces=trail,
                           collapse=collapse, flip2=flip2)


@functools.lru_cache(maxsize=None)
def relaxed_input(name):
    """The oracle's split-and-flipped mesh of ``open_case(name)``: what ``relax_project`` gets in the pipeline."""
    c = open_case(name)
    return c.split[0], c.flip[0]


# ---- the oracles with one rule changed -----------------------------------------------------------------------------------
def round_f32(q):
    """The float32 nearest to the rational ``q``, ties to even (no overflow handling: the fixtures are small)."""
    q = Fraction(q)
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                             # 2^e <= q < 2^(e + 1)
    shift = max(e, -126) - 23
    m = q / Fraction(2) ** shift
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * math.ldexp(n, shift))


def len2_fused(vs, lo, hi):
    """``fma(dz, dz, fma(dy, dy, dx * dx))``: what a compiler that contracts makes of ``RO.len2``.  Each fma is evaluated
    exactly and rounded once."""
    d = [np.float32(vs[hi][i]) - np.float32(vs[lo][i]) for i in range(3)]
    acc = np.float32(d[0] * d[0])
    for k in (1, 2):
        acc = round_f32(Fraction(float(d[k])) ** 2 + Fraction(float(acc)))
    return acc


def _dot_zero_passes(u, v, _dot=RO._dot):
    """``_dot`` for a guard written ``>= 0``: an exact zero is handed on as the smallest positive number."""
    d = _dot(u, v)
    return d if d != 0.0 else 5e-324


@contextlib.contextmanager
def altered(border=None, zero_passes=False, fused=False, guard_log=None):
    """The oracles with a rule changed while the block runs.  ``border``: a function (true border set, faces) -> the set the
    flip uses; ``zero_passes``: both fold-over guards accept a dot product of exactly 0; ``fused``: ``len2`` is
    ``len2_fused``; ``guard_log``: a list that receives the outcome of every evaluation of the flip guard (nothing changes)."""
    keep = (RO.valences, RO._dot, CO._dot, RO.len2, CO.len2, RO.guard)
    if border is not None:
        def valences(faces, _orig=RO.valences):
            val, true_border = _orig(faces)
            return val, set(border(true_border, faces))
        RO.valences = valences
    if zero_passes:
        RO._dot = CO._dot = _dot_zero_passes
    if fused:
        RO.len2 = CO.len2 = len2_fused
    if guard_log is not None:
        def guard(vs, a, b, c, d, _orig=RO.guard):
            ok = _orig(vs, a, b, c, d)
            guard_log.append(ok)
            return ok
        RO.guard = guard
    try:
        yield
    finally:
        RO.valences, RO._dot, CO._dot, RO.len2, CO.len2, RO.guard = keep


def faces_changed(a, b):
    """The number of face slots in which two face arrays of one shape differ."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    return int((a != b).any(1).sum())


def zero_area_faces(vs, faces):
    """The faces whose area is zero in exact arithmetic on the float32 coordinates."""
    P = [[Fraction(float(x)) for x in p] for p in np.asarray(vs, np.float32)]
    out = []
    for f, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        u = [P[b][i] - P[a][i] for i in range(3)]
        v = [P[c][i] - P[a][i] for i in range(3)]
        if u[1] * v[2] == u[2] * v[1] and u[2] * v[0] == u[0] * v[2] and u[0] * v[1] == u[1] * v[0]:
            out.append(f)
    return out


# ---- guard ties: a dot product of exactly zero ---------------------------------------------------------------------------
def _best_spoke(n):
    """The rim vertex j of a fan (hub 0, rim 1 .. n, spokes of equal gain) whose spoke {0, j} has the highest hash: the
    spokes are the edges of rank 0 .. n - 1."""
    return 1 + max(range(n), key=RO.hash32)


def fan8_on_chord():
    """``RO.fan8()`` with the rim vertex j of the winning spoke moved to the midpoint of the chord between its rim neighbours
    (half-integer coordinates): the flip of {0, j} would make the triangle (j - 1, j, j + 1) of zero area, its normal is
    exactly (0, 0, 0) and the guard's dot products with it are exactly 0.  Returns (vs, faces, j)."""
    vs, faces = RO.fan8()
    j = _best_spoke(8)
    before, after = 1 + (j - 2) % 8, 1 + j % 8
    vs[j] = (vs[before] + vs[after]) * np.float32(0.5)
    return vs, faces, j


def fan8_right_angle():
    """The fan's topology with integer coordinates in space: hub (0, 0, 0), j at (0, 2, 0), the next rim vertex at
    (-1, 1, 0) and the one before at (-1, 1, 1), straight above it.  The new triangle (0, j - 1, j + 1) stands upright on the
    plane of (0, j, j + 1): normals (-1, -1, 0) and (0, 0, 2), dot product exactly 0, no triangle degenerate.  The other five
    rim vertices keep the octagon's places (rotated so that j sits where it does).  Returns (vs, faces, j)."""
    _, faces = RO.fan8()
    j = _best_spoke(8)
    ring = [(0, 2, 0), (-1, 1, 0), (-2, -1, 0), (-1, -2, 0), (1, -2, 0), (2, -1, 0), (2, 1, 0), (-1, 1, 1)]   # j, j + 1, ...
    vs = np.zeros((9, 3), np.float32)
    for i, p in enumerate(ring):
        vs[1 + (j - 1 + i) % 8] = p
    return vs, faces, j


def fan7_collinear():
    """A hub (vertex 0) with seven rim vertices, planar, integer coordinates.  Spoke {0, 1} is the shortest edge (len2 1), so the
    collapse's first candidate is hub -> vertex 1; vertex 1 = (0, 1) lies on the line through rim vertices 2 and 3, so the face
    (0, 2, 3) would become (1, 2, 3) with zero area: the collapse's fold-over dot product is exactly 0 there and positive for
    the other faces."""
    rim = [(0, 1), (-2, 2), (-4, 3), (-3, -2), (0, -3), (3, -2), (3, 2)]
    vs = np.array([(0, 0, 0)] + [(x, y, 0) for x, y in rim], np.float32)
    faces = np.array([(0, 1 + i, 1 + (i + 1) % 7) for i in range(7)], np.int64)
    return vs, faces


GUARD_TIES = {"fan8_on_chord": lambda: fan8_on_chord()[:2], "fan8_right_angle": lambda: fan8_right_angle()[:2],
              "fan7_collinear": fan7_collinear}
#: the target at which every edge of the guard-tie fixtures is short and no length guard holds (as tests/test_gpu_collapse.py)
GUARD_TIE_TARGET = 10.0


# ---- threshold ties: one edge per component within one ulp of a threshold ----------------------------------------------------
TIE_TARGET = 0.7
_H_SHORT = math.sqrt(0.8 ** 2 - 2 * 0.3 ** 2)
_SIDE = 4.0 / 3.0 / math.sqrt(2.0)
_H_GUARD = math.sqrt(0.7 ** 2 - 2 * 0.25 ** 2)
_PYRAMID_FACES = [(4, 0, 1), (4, 1, 2), (4, 2, 3), (4, 3, 0)]
#: name -> (local coordinates in units of the target with vertex 0 at the origin, faces, the tied edge, which threshold, the
#: comparison the stage makes).  "split": single triangles, the tied edge at 4/3 target, the other two at 0.72 target.
#: "short": a pyramid over a square of side 0.9 (diagonal 1.27 < 4/3) whose apex is 0.8 from corner 0 and at least 0.95 from the
#: others: spoke {0, 4} is the only edge near lo2, the rim edges have one face, and the collapse apex -> corner 0 passes every
#: guard with a margin.  "guard": the same with the spoke clearly short (0.7) and the square's diagonal {0, 2} at 4/3: the one
#: candidate stands or falls with ``len2(k, w) > thr2``.
TIE_SOUPS = {
    "split": (np.array([(0, 0, 0), (4 / 3, 0, 0), (2 / 3, 4 / 15, 0)]), [(0, 1, 2)], (0, 1), "thr2", np.greater),
    "short": (np.array([(0, 0, 0), (0.9, 0, 0), (0.9, 0.9, 0), (0, 0.9, 0), (0.3, 0.3, _H_SHORT)]), _PYRAMID_FACES, (0, 4), "lo2",
              np.less),
    "guard": (np.array([(0, 0, 0), (_SIDE, 0, 0), (_SIDE, _SIDE, 0), (0, _SIDE, 0), (0.25, 0.25, _H_GUARD)]), _PYRAMID_FACES,
              (0, 2), "thr2", np.greater),
}
_TRIES, _CELLS = 120000, 512
_QUOTA = {"discordant": 96, "exact": 16, "near": 16}


def _len2_rows(a, b):
    """``RO.len2`` on rows of float32 arrays: numpy rounds every array operation to float32."""
    d = b - a
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _frames(a, b):
    """Orthonormal frames (e1, e2, e3), rows of [N, 3] arrays, from two random vectors each by Gram-Schmidt, written out in
    single multiplies, adds, divides and square roots: the same bits on every machine, whatever its linear algebra library."""
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    e1 = a / np.sqrt(dot(a, a))[:, None]
    b = b - dot(b, e1)[:, None] * e1
    e2 = b / np.sqrt(dot(b, b))[:, None]
    e3 = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return e1, e2, e3


@functools.lru_cache(maxsize=None)
def tie_soup(name, seed=2025):
    """(vs, faces, info): disconnected copies of the component ``TIE_SOUPS[name]``, each in a random attitude in its own cell of
    an 8 x 8 x 8 lattice of spacing 2, scaled so that the tied edge's ``len2`` lands within one ulp of the threshold.  A seeded
    search keeps, first come first kept and one per cell, up to 96 components whose fused and unfused ``len2`` fall on
    different sides of the comparison (*discordant*), 16 whose unfused ``len2`` equals the threshold and 16 further near ones.
    ``info``: per component the tied edge (vertex ids), its unfused and fused ``len2`` and its kind; and the threshold."""
    local, faces, pair, which, compare = TIE_SOUPS[name]
    thr = {"thr2": RO.split_threshold, "lo2": CO.collapse_threshold}[which](TIE_TARGET)
    rng = np.random.default_rng(seed)
    n = local.shape[0]
    e1, e2, e3 = _frames(rng.normal(size=(_TRIES, 3)), rng.normal(size=(_TRIES, 3)))
    cell = np.arange(_TRIES) % _CELLS
    origin = 2.0 * np.stack(np.unravel_index(cell, (8, 8, 8)), 1) + 0.5 * rng.random((_TRIES, 3))
    scale = TIE_TARGET * (1.0 + rng.uniform(-3e-6, 3e-6, _TRIES))
    pts = np.stack([origin + (e1 * float(x) + e2 * float(y) + e3 * float(z)) * scale[:, None] for x, y, z in local], 1).astype(np.float32)
    l2 = _len2_rows(pts[:, pair[0]], pts[:, pair[1]])
    near = np.abs(l2.view(np.int32).astype(np.int64) - RO.bits(thr)) <= 1
    taken, kept, quota = set(), [], dict(_QUOTA)
    for t in np.flatnonzero(near):
        if cell[t] in taken or not any(quota.values()):
            continue
        fused = len2_fused(pts[t], *pair)
        kind = "discordant" if bool(compare(l2[t], thr)) != bool(compare(fused, thr)) else ("exact" if l2[t] == thr else "near")
        if quota[kind]:
            quota[kind] -= 1
            taken.add(cell[t])
            kept.append((t, kind, fused))
    kept.sort(key=lambda k: cell[k[0]])
    vs = np.concatenate([pts[t] for t, _, _ in kept]).astype(np.float32)
    all_faces = np.concatenate([np.asarray(faces, np.int64) + n * i for i in range(len(kept))])
    info = SimpleNamespace(threshold=thr, which=which, compare=compare, n_components=len(kept),
                           edges=np.array([[n * i + pair[0], n * i + pair[1]] for i in range(len(kept))]),
                           unfused=np.array([l2[t] for t, _, _ in kept], np.float32),
                           fused=np.array([f for _, _, f in kept], np.float32), kinds=[k for _, k, _ in kept])
    vs.setflags(write=False)
    all_faces.setflags(write=False)
    return vs, all_faces, info
