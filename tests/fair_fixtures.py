"""The meshes the thin-plate fairing tests share, in numpy: small open meshes, their raw fill by tests/holes_oracle.py and the
mask of the inserted vertices.  Everything is computed once and handed out read-only.

  a  square hole (n = 4: the two faces of one quad) in a 6 x 6 planar grid          one free vertex, the fan centre
  b  icosphere of 642 vertices minus a 2-ring disc
  c  the same minus a 3-ring disc
  d  ``holes.cut_torus(24, 48, 3)`` restated in numpy                                 three free classes
  e  a 14 x 9 grid with a hole of 12 edges next to one of 18 that ``max_hole_edges = 12`` leaves open (and so the outer
     border): rows of S one edge from a border
  f  a 9 x 9 grid whose hole has an ear: a loop vertex with one mesh face, valence 3 once the patch is in

The second family (``masked``) has no fill: a mesh, a mask of the caller's and start positions off the minimiser.

  sweep<k>    64 x 64 grid with a smooth height; free = the first k vertices (ascending id) of the disc of radius 20.3
              round the grid's centre, k in SWEEP: one wavefront, one block and one partial more or less than full
  disc        that whole disc: 1288 free vertices, six blocks, the last one partial
  blocks      861 x 861 grid; free where i % 5 and j % 5 are both in {1, 2, 3}: 266 256 free vertices (more than 1024
              blocks of 256) in 29 584 classes of 9 that share no row, so A is block diagonal (``blocks_exact``)
  sphere_mask, grid_mask      a seeded 30 % mask on icosphere(2) and on an open 12 x 12 grid, border vertices included
  wheel_hub, wheel_rim        a wheel of 40 spokes with the hub free (valence 40), and with the rim free (valence 3)
  soup, soup_clean            a grid with a fin (one edge with three faces); the soup repeats faces, some of them reversed
  plane_off, plane_in         24 x 24 grid in z = 0, 232 free vertices in a disc, started 0.3 off their places in all three
                              coordinates (b = 0 but r0 != 0 in z), and in x and y only (b = 0 and r0 = 0 in z)
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


# ---- meshes with a mask of the caller's ----------------------------------------------------------------------------------
@dataclass(frozen=True)
class Masked:
    vs: np.ndarray                   # float32 [V, 3]
    faces: np.ndarray                # int64 [F, 3]
    free: np.ndarray                 # bool [V]


SWEEP = (63, 64, 65, 255, 256, 257, 513, 1025)
BLOCKS_N, BLOCKS_PERIOD = 861, 5
MASKS = ("sphere_mask", "grid_mask", "wheel_hub", "wheel_rim", "soup")
PLANES = ("plane_off", "plane_in")
SMALL = tuple(f"sweep{k}" for k in SWEEP) + ("disc",) + MASKS + ("soup_clean",) + PLANES      # within reach of FO.System


def grid_faces(n, m):
    """the faces of ``grid(n, m)``, without the loop"""
    a, b = np.meshgrid(np.arange(n - 1), np.arange(m - 1), indexing="ij")
    v00 = (a * m + b).ravel()
    v10, v11, v01 = v00 + m, v00 + m + 1, v00 + 1
    return np.stack([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)], 1).reshape(-1, 3).astype(np.int64)


def height_grid(n, amplitude):
    """n x n grid at integer x, y with the height ``amplitude (sin(3.1 i / n) cos(2.3 j / n) + 1.5)``"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = i.ravel().astype(np.float64), j.ravel().astype(np.float64)
    z = amplitude * (np.sin(3.1 * i / n) * np.cos(2.3 * j / n) + 1.5)
    return np.stack([i, j, z], 1), grid_faces(n, n)


def centre_disc(n, radius):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return ((i - (n - 1) / 2) ** 2 + (j - (n - 1) / 2) ** 2 <= radius * radius).ravel()


def _masked(vs, faces, free, noise=0.0, seed=0, columns=(0, 1, 2)):
    """The free vertices moved by seeded uniform noise of that size in ``columns``; everything rounded to float32 once."""
    vs = np.array(vs, np.float64)
    free = np.asarray(free, bool)
    if noise:
        step = np.random.default_rng(seed).uniform(-noise, noise, (int(free.sum()), 3))
        for c in columns:
            vs[free, c] += step[:, c]
    out = Masked(np.ascontiguousarray(vs.astype(np.float32)), np.ascontiguousarray(np.asarray(faces, np.int64)), free)
    for a in (out.vs, out.faces, out.free):
        a.setflags(write=False)
    return out


def wheel(spokes):
    """hub 0 above a rim 1 .. spokes that undulates round (1.5, 1, 1): no coordinate of a minimiser is near 0, where the
    direct solve's own rounding would be all there is to compare with; faces (hub, k, k + 1)"""
    a = 2 * np.pi * np.arange(spokes) / spokes
    rim = np.stack([1.5 + np.cos(a), 1.0 + np.sin(a), 1.0 + 0.2 * np.sin(3 * a)], 1)
    k = np.arange(spokes)
    faces = np.stack([np.zeros(spokes, np.int64), 1 + k, 1 + (k + 1) % spokes], 1)
    return np.concatenate([[[1.625, 0.75, 1.5]], rim], 0), faces


def fin_grid():
    """7 x 7 grid with a height, and one more face on the interior edge (3, 3)-(4, 4): that edge has three faces"""
    vs, faces = height_grid(7, 0.5)
    vs = np.concatenate([vs, [[3.4, 3.6, 2.0]]], 0)
    return vs, np.concatenate([faces, [[3 * 7 + 3, 4 * 7 + 4, 49]]], 0)


@functools.lru_cache(maxsize=None)
def masked(name) -> Masked:
    if name.startswith("sweep") or name == "disc":
        vs, faces = height_grid(64, 4.0)
        disc = centre_disc(64, 20.3)
        k = int(disc.sum()) if name == "disc" else int(name[5:])
        free = np.zeros(64 * 64, bool)
        free[np.flatnonzero(disc)[:k]] = True
        return _masked(vs, faces, free, 0.3, seed=k)
    if name == "blocks":
        n, q = BLOCKS_N, BLOCKS_PERIOD
        vs, faces = height_grid(n, 4.0)
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        free = (np.isin(i % q, (1, 2, 3)) & np.isin(j % q, (1, 2, 3))).ravel()
        return _masked(vs, faces, free, 0.3, seed=q)
    if name == "sphere_mask":
        vs, faces = icosphere(2)
        return _masked(vs, faces, np.random.default_rng(21).random(len(vs)) < 0.3, 0.1, seed=22)
    if name == "grid_mask":
        vs, faces = height_grid(12, 1.0)
        return _masked(vs, faces, np.random.default_rng(23).random(144) < 0.3, 0.3, seed=24)
    if name in ("wheel_hub", "wheel_rim"):
        vs, faces = wheel(40)
        free = np.arange(41) == 0
        return _masked(vs, faces, free if name == "wheel_hub" else ~free, 0.1, seed=25)
    if name in ("soup", "soup_clean"):
        vs, faces = fin_grid()
        free = np.zeros(50, bool)
        free[[2 * 7 + 2, 2 * 7 + 3, 3 * 7 + 3, 4 * 7 + 4, 4 * 7 + 3, 49]] = True        # both ends of the fin's edge, and its tip
        if name == "soup":
            rng = np.random.default_rng(26)
            again, back = rng.choice(len(faces), 9, replace=False), rng.choice(len(faces), 7, replace=False)
            faces = np.concatenate([faces, faces[again], faces[back][:, ::-1], faces[-1:], faces[-1:, ::-1]], 0)
            faces = faces[rng.permutation(len(faces))]
        return _masked(vs, faces, free, 0.3, seed=27)
    if name in PLANES:
        vs, faces = grid(24, 24)
        return _masked(vs, faces, centre_disc(24, 8.6), 0.3, seed=28, columns=(0, 1, 2) if name == "plane_off" else (0, 1))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def table(name) -> FO.Table:
    c = masked(name) if name not in NAMES else case(name)
    return FO.Table(c.faces, len(c.vs))


@functools.lru_cache(maxsize=None)
def masked_system(name) -> FO.System:
    assert name in SMALL
    c = masked(name)
    return FO.System(c.vs, c.faces, c.free)


@dataclass(frozen=True)
class BlocksExact:
    A: np.ndarray                    # float64 [B, 9, 9]  the diagonal blocks of A
    rows: np.ndarray                 # int64 [B, 9]       their free indices
    b: np.ndarray                    # float64 [nf, 3]
    x: np.ndarray                    # float64 [nf, 3]    the solution of every block
    min_eig: float                   # the smallest eigenvalue over all blocks


@functools.lru_cache(maxsize=None)
def blocks_exact() -> BlocksExact:
    """The blocks fixture solved class by class.  Two free vertices couple in A exactly when a row holds both, and no row
    of this mask reaches two classes, so ``A`` applied to the indicator of one of the nine places of a class, read at the
    class's own vertices, is a column of that class's 9 x 9 block."""
    c, t = masked("blocks"), table("blocks")
    n, q = BLOCKS_N, BLOCKS_PERIOD
    ids = np.flatnonzero(c.free)
    i, j = ids // n, ids % n
    place = (i % q - 1) * 3 + (j % q - 1)
    block = (i // q) * ((n + q - 1) // q) + j // q
    order = np.lexsort((place, block))
    rows = order.reshape(-1, 9)
    assert (block[rows] == block[rows[:, :1]]).all() and (place[rows] == np.arange(9)).all()
    cols = FO.apply_table(t, c.free, (place[:, None] == np.arange(9)).astype(np.float64))       # [nf, 9]
    A = cols[rows]                                           # A[B, r, k] = (A e_k)[row r of B]
    b = -FO.normal_rows(t, c.free, c.vs, True)
    x = np.empty_like(b)
    x[rows.reshape(-1)] = np.linalg.solve(A, b[rows]).reshape(-1, 3)
    return BlocksExact(A, rows, b, x, float(np.linalg.eigvalsh(0.5 * (A + A.transpose(0, 2, 1))).min()))
