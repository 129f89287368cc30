"""The meshes the thin-plate fairing tests share, in numpy: small open meshes, their raw fill by tests/holes_oracle.py and the
mask of the inserted vertices.  Everything is computed once and handed out read-only.

  a  square hole (n = 4: the two faces of one quad) in a 6 x 6 planar grid          one free vertex, the fan centre
  b  icosphere of 642 vertices minus a 2-ring disc
  c  the same minus a 3-ring disc
  d  ``holes.cut_torus(24, 48, 3)`` restated in numpy                                 three free classes
  e  a 14 x 9 grid with a hole of 12 edges next to one of 18 that ``max_hole_edges = 12`` leaves open (and so the outer
     border): rows of S one edge from a border
  f  a 9 x 9 grid whose hole has an ear: a loop vertex with one mesh face, valence 3 once the patch is in
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

import fair_oracle as FO
import holes_oracle as HO


@dataclass(frozen=True)
class Case:
    open_vs: np.ndarray              # float32 [V, 3]   the mesh with its holes
    open_faces: np.ndarray           # int64 [F, 3]
    max_hole_edges: Optional[int]
    vs: np.ndarray                   # float32 [V + Vn, 3]  the raw fill (the oracle's float64 positions rounded once)
    faces: np.ndarray                # int64 [F + Fn, 3]
    free: np.ndarray                 # bool [V + Vn]    the inserted vertices

    @property
    def V(self):
        return self.open_vs.shape[0]


def compact(vs, faces):
    used = np.zeros(vs.shape[0], bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return np.ascontiguousarray(vs[used].astype(np.float32)), np.ascontiguousarray(new_id[faces].astype(np.int64))


def within(faces, V, seeds, rings):
    """bool [V]: the vertices at most ``rings`` edges from a seed."""
    N = FO.neighbours(faces, V)
    mask = np.zeros(V, bool)
    mask[np.asarray(seeds, np.int64)] = True
    for _ in range(rings):
        grown = mask.copy()
        for i in np.flatnonzero(mask):
            grown[N[i]] = True
        mask = grown
    return mask


def cut(vs, faces, seeds, rings):
    """Drop the faces that touch a vertex within ``rings`` rings of a seed, then the unused vertices."""
    hole = within(faces, vs.shape[0], seeds, rings)
    return compact(vs, faces[~hole[faces].any(1)])


def grid(n, m, tilt=False):
    """Open n x m grid, every quad cut along the same diagonal (interior valence 6): in the plane z = 0, or with ``tilt`` in
    the plane through the origin spanned by (1, 0.25, 0.5) and (-0.125, 1, 0.75)."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    i, j = i.ravel().astype(np.float64), j.ravel().astype(np.float64)
    if tilt:
        vs = i[:, None] * np.array([1.0, 0.25, 0.5]) + j[:, None] * np.array([-0.125, 1.0, 0.75])
    else:
        vs = np.stack([i, j, np.zeros(n * m)], 1)
    faces = []
    for a in range(n - 1):
        for b in range(m - 1):
            v00, v10, v11, v01 = a * m + b, (a + 1) * m + b, (a + 1) * m + b + 1, a * m + b + 1
            faces += [[v00, v10, v11], [v00, v11, v01]]
    return vs.astype(np.float32), np.asarray(faces, np.int64)


TILT_NORMAL = np.cross([1.0, 0.25, 0.5], [-0.125, 1.0, 0.75])


def icosphere(level=3):
    """The icosahedron subdivided ``level`` times on the unit sphere: 10 * 4^level + 2 vertices (642 at level 3)."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    vs = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                   [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    faces = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                      [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                      [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    for _ in range(level):
        V = vs.shape[0]
        e = np.sort(np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 1).reshape(-1, 2), 1)
        key, inv = np.unique(e[:, 0] * V + e[:, 1], return_inverse=True)
        mid = 0.5 * (vs[key // V] + vs[key % V])
        m = V + inv.reshape(-1, 3)
        vs = np.concatenate([vs, mid], 0)
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        faces = np.concatenate([np.stack([a, m[:, 0], m[:, 2]], 1), np.stack([m[:, 0], b, m[:, 1]], 1),
                                np.stack([m[:, 2], m[:, 1], c], 1), m], 0)
    vs = vs / np.linalg.norm(vs, axis=1, keepdims=True)
    return vs.astype(np.float32), faces


def cut_torus_np(nu, nv, n_discs, frac=0.05):
    """``semigcn_amd.holes.cut_torus`` without a device: the same seeds, the same ring count, the same compaction."""
    from semigcn_amd import synth
    m = synth.torus_mesh(nu, nv, masks=False)
    V = m.num_vertices
    target = frac * V / max(n_discs, 1)
    rings = max(1, int(round((math.sqrt(max(12 * target - 3, 0.0)) - 3) / 6)))
    gu = max(1, int(math.ceil(math.sqrt(n_discs * nu / nv))))
    gv = max(1, int(math.ceil(n_discs / gu)))
    cells = [(a, b) for a in range(gu) for b in range(gv)][:n_discs]
    seeds = [((a * nu) // gu + nu // (2 * gu)) * nv + (b * nv) // gv + nv // (2 * gv) for a, b in cells]
    return cut(m.vs.astype(np.float32), m.faces, seeds, rings)


def _case(open_vs, open_faces, max_hole_edges=None):
    vs, faces, inserted, _filled, _loops = HO.fill_holes(open_vs, open_faces, max_hole_edges)
    out = Case(open_vs, open_faces, max_hole_edges, np.ascontiguousarray(vs.astype(np.float32)), faces, inserted)
    for a in (out.open_vs, out.open_faces, out.vs, out.faces, out.free):
        a.setflags(write=False)
    return out


def square_hole(tilt=False):
    vs, faces = grid(6, 6, tilt)
    keep = np.ones(len(faces), bool)
    keep[2 * (2 * 5 + 2): 2 * (2 * 5 + 2) + 2] = False            # the quad (2, 2) .. (3, 3)
    return compact(vs, faces[keep])


def sphere_cap(rings):
    vs, faces = icosphere(3)
    return cut(vs, faces, [200], rings)


def two_holes(tilt=False):
    vs, faces = grid(14, 9, tilt)
    return cut(*cut(vs, faces, [3 * 9 + 4], 1), [_grid_id_after_cut(14, 9, (3, 4), 1, (9, 4))], 2)


def _grid_id_after_cut(n, m, centre, rings, vertex):
    """id of grid vertex ``vertex`` once the disc of ``rings`` rings round ``centre`` has been compacted away"""
    _vs, faces = grid(n, m)
    gone = within(faces, n * m, [centre[0] * m + centre[1]], rings)
    assert not gone[vertex[0] * m + vertex[1]]
    return int((np.cumsum(~gone) - 1)[vertex[0] * m + vertex[1]])


def ear_hole():
    """The hole of 12 edges of a 9 x 9 grid, made larger by the faces round one of its loop vertices but one: the first
    choice (loop order, then face order) that leaves the boundary orderable and gives that vertex valence 3 once the patch
    is in."""
    vs, faces = cut(*grid(9, 9), [4 * 9 + 4], 1)
    loop = HO.boundary_loops(faces)
    loop = next(l for l in loop if len(l) == 12)
    for v in loop:
        for keep in np.flatnonzero((faces == v).any(1)):
            drop = (faces == v).any(1)
            drop[keep] = False
            try:
                o_vs, o_faces = compact(vs, faces[~drop])
                f_vs, f_faces, inserted, _f, loops = HO.fill_holes(o_vs, o_faces, 20)
            except (HO.Unorderable, KeyError):
                continue
            d = np.array([len(n) for n in FO.neighbours(f_faces, f_vs.shape[0])])
            loop_of_patch = [l for l in loops if len(l) <= 20]
            if len(loop_of_patch) == 1 and any(d[u] == 3 for u in loop_of_patch[0]):
                return o_vs, o_faces
    raise AssertionError("no ear found")


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    if name == "a":
        return _case(*square_hole(), max_hole_edges=4)
    if name == "a_tilted":
        return _case(*square_hole(tilt=True), max_hole_edges=4)
    if name == "b":
        return _case(*sphere_cap(2))
    if name == "c":
        return _case(*sphere_cap(3))
    if name == "d":
        return _case(*cut_torus_np(24, 48, 3))
    if name == "e":
        return _case(*two_holes(), max_hole_edges=12)
    if name == "e_tilted":
        return _case(*two_holes(tilt=True), max_hole_edges=12)
    if name == "f":
        return _case(*ear_hole(), max_hole_edges=20)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def system(name) -> FO.System:
    c = case(name)
    return FO.System(c.vs, c.faces, c.free)


NAMES = ("a", "b", "c", "d", "e", "f")
