"""Fixtures of the simplify stage, shared by tests/test_simplify_oracle.py (their premises, on the CPU) and
tests/test_gpu_simplify.py (the device).  Everything here is numpy and the serial oracle (tests/simplify_oracle.py); nothing
is shared with the kernels.  ``case(name, ratio, quadrics)`` runs the oracle once per process and hands out read-only
arrays."""
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


@functools.lru_cache(maxsize=None)
def mesh(name):
    vs, faces = FIXTURES[name]()
    vs, faces = np.ascontiguousarray(vs, np.float32), np.ascontiguousarray(faces, np.int64)
    vs.setflags(write=False)
    faces.setflags(write=False)
    return vs, faces


@functools.lru_cache(maxsize=None)
def case(name, ratio, quadrics="own", guard=True):
    vs, faces = mesh(name)
    target = int(vs.shape[0] * ratio)
    out = SO.simplify(vs, faces, target, quadrics=quadrics, guard=guard)
    for a in out[:4]:
        a.setflags(write=False)
    return SimpleNamespace(name=name, in_vs=vs, in_faces=faces, target=target, vs=out[0], faces=out[1], vertex_ids=out[2],
                           coarse_of=out[3], counts=out[4], reached=out[5], refused=out[6])


def edge_counts(faces):
    """{(lo, hi): number of faces}"""
    return {e: len(hs) for e, hs in RO.edge_table(faces)[0].items()}


def euler(vs, faces):
    return vs.shape[0] - len(edge_counts(faces)) + faces.shape[0]
