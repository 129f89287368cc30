"""What "two faces cross" MEANS, in exact rational arithmetic: the truth tests/intersect_oracle.py and the device are
held to.  This is the definition, not the predicate of semigcn_amd/repair.py: there is no orient3d / orient2d sign
cascade, no projection, no drop axis and no branch on which edge or which slot.  It imports nothing from the restatement.

Two non-degenerate faces A and B are closed triangles.  A is clipped as a polygon (Sutherland-Hodgman) against the closed
half-spaces ``n.x >= d`` and ``n.x <= d`` of B's plane and ``(n x e_k).(x - p_k) >= 0`` of B's three edges; every
intersection point is a ``fractions.Fraction`` triple.  What is left is the vertex set R of the convex set A n B: empty, a
point, a segment or a polygon.  The verdict then depends only on the vertex ids the faces share:

* all three: a pair (a duplicate);
* none: a pair when R is not empty;
* one, S: a pair when some point of R is not S;
* two, U and V: a pair when some point of R does not lie on the closed segment UV.

A face with a repeated id or an exactly zero rational normal takes part in nothing.

Coordinates are read as the exact rationals they are: Python / numpy integers, or floats (a float32 or float64 value is a
dyadic rational; ``Fraction`` takes it without rounding).  Only the box prefilter of ``self_intersections_exact`` uses
numpy, with comparisons of the stored values, which are exact.  About a millisecond per pair: for test inputs only."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def points(vs):
    """vs [V, 3] (integer or float) as a list of exact Fraction triples."""
    vs = np.asarray(vs)
    if np.issubdtype(vs.dtype, np.integer):
        return [tuple(Fraction(int(x)) for x in row) for row in vs.reshape(-1, 3)]
    return [tuple(Fraction(float(x)) for x in row) for row in vs.reshape(-1, 3)]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def normal(P, f):
    """The exact normal (b - a) x (c - a) of the face with ids f."""
    a, b, c = P[f[0]], P[f[1]], P[f[2]]
    return _cross(_sub(b, a), _sub(c, a))


def degenerate(P, f):
    return f[0] == f[1] or f[1] == f[2] or f[2] == f[0] or normal(P, f) == (0, 0, 0)


def _clip(poly, g, origin, sign=1):
    """The vertices of conv(poly) with sign g.(x - origin) >= 0.  ``poly`` lists the vertices of a convex set in cyclic
    order; one and two vertices (a point, a segment) are polygons too."""
    h = [sign * _dot(g, _sub(p, origin)) for p in poly]
    n = len(poly)
    if n <= 1:
        return [p for p, hp in zip(poly, h) if hp >= 0]
    out = []
    for k in range(n if n > 2 else 1):                     # a segment has one edge, not two
        p, q, hp, hq = poly[k], poly[(k + 1) % n], h[k], h[(k + 1) % n]
        if hp >= 0:
            out.append(p)
        if (hp > 0 and hq < 0) or (hp < 0 and hq > 0):
            t = hp / (hp - hq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]), p[2] + t * (q[2] - p[2])))
    if n == 2 and h[1] >= 0:
        out.append(poly[1])
    seen, uniq = set(), []
    for p in out:                                          # the same point once: the order of the rest is kept
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def common_part(P, fa, fb):
    """The vertex set of (closed triangle fa) n (closed triangle fb); both non-degenerate."""
    b = [P[fb[0]], P[fb[1]], P[fb[2]]]
    n = _cross(_sub(b[1], b[0]), _sub(b[2], b[0]))
    poly = [P[fa[0]], P[fa[1]], P[fa[2]]]
    poly = _clip(poly, n, b[0], 1)
    poly = _clip(poly, n, b[0], -1)
    for k in range(3):
        if not poly:
            break
        poly = _clip(poly, _cross(n, _sub(b[(k + 1) % 3], b[k])), b[k], 1)
    return poly


def _on_segment(p, u, v):
    d, w = _sub(v, u), _sub(p, u)
    if _cross(d, w) != (0, 0, 0):
        return False
    t = _dot(d, w)
    return 0 <= t <= _dot(d, d)


def crosses(P, fa, fb):
    """Whether the faces with ids fa and fb (of the exact points P) are a pair."""
    fa, fb = [int(x) for x in fa], [int(x) for x in fb]
    if degenerate(P, fa) or degenerate(P, fb):
        return False
    shared = sorted(set(fa) & set(fb))
    if len(shared) == 3:
        return True
    R = common_part(P, fa, fb)
    if len(shared) == 0:
        return len(R) > 0
    if len(shared) == 1:
        return any(p != P[shared[0]] for p in R)
    return any(not _on_segment(p, P[shared[0]], P[shared[1]]) for p in R)


def candidates(vs, faces, chunk=256):
    """(i, j), i < j, of all faces whose closed boxes meet, in lexicographic order (comparisons of the stored values)."""
    vs, faces = np.asarray(vs).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    T = vs[faces]
    lo, hi = T.min(1), T.max(1)
    F = faces.shape[0]
    out = [np.zeros((0, 2), np.int64)]
    for s in range(0, F, chunk):
        e = min(s + chunk, F)
        meet = ((lo[s:e, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[s:e, None, :])).all(2)
        meet &= np.arange(F)[None, :] > np.arange(s, e)[:, None]
        i, j = np.nonzero(meet)
        out.append(np.stack([i + s, j], 1))
    return np.concatenate(out)


def self_intersections_exact(vs, faces):
    """(pairs int64 [P, 2] with i < j in lexicographic order, n_degenerate) by the definition above."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = points(vs)
    rows = faces.tolist()
    bad = np.array([degenerate(P, f) for f in rows], bool).reshape(-1)
    cand = candidates(vs, faces)
    cand = cand[~bad[cand[:, 0]] & ~bad[cand[:, 1]]]
    hit = [crosses(P, rows[i], rows[j]) for i, j in cand.tolist()]
    return cand[np.asarray(hit, bool).reshape(-1)].reshape(-1, 2), int(bad.sum())
