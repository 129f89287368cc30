"""Meshes and poses of the registration tests (semigcn_amd/align.py), all float32 / int64 numpy.

``E_O``: the largest distance between ``align_oracle.transform(matrix, source)`` and the target's vertices after
``align_oracle.align_loop`` on the lumpy torus, its vertices under ``similarity()`` as the source, with the float64
closest-point oracle (tests/mesh_distance_oracle.py) as the query: measured 1.69e-7 with scale and 1.37e-7 without, four
iterations each (tests/test_align_oracle.py prints both).  It is the rounding of the float32 coordinates (|x| up to 3.4, half
a unit in the last place 1.2e-7 per coordinate, in the source and again in the transformed points), not a residual of the
iteration: the recovered matrix itself is within 1.1e-8 of the inverse of the similarity.  The device tests allow 4 * E_O."""
from __future__ import annotations

import numpy as np

import align_oracle as AO

E_O = 1.7e-7


def lumpy_torus(nu: int = 20, nv: int = 10):
    """A closed torus of ``nu`` x ``nv`` vertices (V = nu nv, F = 2 nu nv; 200 and 400 by default) whose tube radius and
    height vary with both angles, so that no rotation, reflection or shift of the angles maps it onto itself."""
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th, ph = 2 * np.pi * u.ravel() / nu, 2 * np.pi * v.ravel() / nv
    r = 0.7 * (1.0 + 0.22 * np.sin(3 * th + 0.5) * np.cos(ph) + 0.15 * np.cos(2 * th - 1.0) + 0.12 * np.sin(ph + 2 * th))
    R = 2.0 + 0.18 * np.sin(th + 0.3) + 0.1 * np.cos(2 * th)
    vs = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th),
                   r * np.sin(ph) + 0.2 * np.sin(2 * th + 1.0)], 1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)                                     # noqa: E731
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [[a, b, c], [a, c, d]]
    return vs.astype(np.float32), np.asarray(faces, np.int64)


def tetrahedron():
    vs = np.array([[0.1, 0.0, -0.2], [1.3, 0.2, 0.1], [0.3, 1.1, 0.0], [0.5, 0.4, 1.2]], np.float32)
    return vs, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64)


def flat_grid(n: int = 6):
    """An ``n`` x ``n`` grid of vertices in the plane z = 0: every face normal is (0, 0, 1) exactly, so a rotation about z
    and a shift along x or y leave every residual alone -- the normal equations are singular."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vs = np.stack([i.ravel() * 0.5, j.ravel() * 0.5, np.zeros(n * n)], 1).astype(np.float32)
    faces = []
    for a in range(n - 1):
        for b in range(n - 1):
            p, q, r, s = a * n + b, (a + 1) * n + b, (a + 1) * n + b + 1, a * n + b + 1
            faces += [[p, q, r], [p, r, s]]
    return vs, np.asarray(faces, np.int64)


def cut_faces(vs, faces, fraction: float = 0.3, at: int = 0):
    """``faces`` without the ``fraction`` of them whose centroids are nearest to the centroid of face ``at``: one patch."""
    c = np.asarray(vs, np.float64)[faces].mean(1)
    order = np.argsort(np.linalg.norm(c - c[at], axis=1), kind="stable")
    keep = np.ones(len(faces), bool)
    keep[order[:int(round(fraction * len(faces)))]] = False
    return faces[keep]


def without_ring(faces, vertex: int):
    """``faces`` without those that name ``vertex``."""
    return faces[~(faces == vertex).any(1)]


def similarity(seed=None, with_scale: bool = True):
    """A 4 x 4 similarity.  ``seed`` None: Cayley parameter (0.08, -0.05, 0.1), scale 1.07, translation (0.3, -0.2, 0.15);
    otherwise drawn from the same ranges (|omega_i| <= 0.1, |s - 1| <= 0.08, |t_i| <= 0.3).  ``with_scale`` False: s = 1."""
    if seed is None:
        omega, s, t = np.array([0.08, -0.05, 0.1]), 1.07, np.array([0.3, -0.2, 0.15])
    else:
        rng = np.random.default_rng(seed)
        omega, s, t = rng.uniform(-0.1, 0.1, 3), 1.0 + rng.uniform(-0.08, 0.08), rng.uniform(-0.3, 0.3, 3)
    return AO.matrix_of((s if with_scale else 1.0) * AO.cayley(omega), t)


def moved(matrix, vs):
    """The float32 vertices ``vs`` under ``matrix``, computed in float64 and rounded once."""
    return AO.transform(matrix, vs)
