"""float64 oracle of the point-to-surface query and of the metric of check/dist_check.py:35-67.

The point-triangle distance is the minimum of (a) the distance to the triangle's plane when the projection of the point
falls inside the triangle and (b) the distances to its three edge segments -- deliberately not the Voronoi-region case
analysis of a closest-point kernel.  A zero-area triangle has no inside: its distance is the one to its segments (or its
point).  Exact with pruning: the distance to the triangle whose centroid is nearest bounds the answer, so every
triangle that can beat it has its centroid within that bound plus the largest centroid-to-vertex radius
(scipy.spatial.cKDTree)."""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree


def _seg(p, s0, s1):
    """closest points of the segments s0 s1 [K,3] to p [3] (a zero-length segment is its point)."""
    d = s1 - s0
    dd = (d * d).sum(1)
    t = np.where(dd > 0, ((p - s0) * d).sum(1) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return s0 + t[:, None] * d


def point_triangles(p, A, B, C):
    """Distances from p [3] to the triangles (A, B, C) [K,3] in float64: (dist [K], closest [K,3], inside [K] -- the
    closest point is interior to the triangle, side [K] = dot((B-A) x (C-A), p - closest))."""
    p = np.asarray(p, np.float64)
    A, B, C = (np.asarray(x, np.float64).reshape(-1, 3) for x in (A, B, C))
    best = None
    for s0, s1 in ((A, B), (B, C), (C, A)):
        c = _seg(p, s0, s1)
        d = np.linalg.norm(p - c, axis=1)
        if best is None:
            best_d, best_c = d, c
            best = True
        else:
            m = d < best_d
            best_d, best_c = np.where(m, d, best_d), np.where(m[:, None], c, best_c)
    n = np.cross(B - A, C - A)
    nn = (n * n).sum(1)
    ok = nn > 0
    nns = np.where(ok, nn, 1.0)
    h = ((p - A) * n).sum(1) / nns
    proj = p - h[:, None] * n
    u = (np.cross(proj - A, C - A) * n).sum(1) / nns
    v = (np.cross(B - A, proj - A) * n).sum(1) / nns
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    d_in = np.abs(h) * np.sqrt(nns)
    inside &= d_in <= best_d
    dist = np.where(inside, d_in, best_d)
    closest = np.where(inside[:, None], proj, best_c)
    side = ((p - closest) * n).sum(1)
    return dist, closest, inside, side


class SurfaceOracle:
    def __init__(self, vs, faces):
        self.vs = np.asarray(vs, np.float64)
        self.faces = np.asarray(faces, np.int64)
        self.A, self.B, self.C = (self.vs[self.faces[:, k]] for k in range(3))
        self.cent = (self.A + self.B + self.C) / 3.0
        self.rmax = float(max(np.linalg.norm(X - self.cent, axis=1).max() for X in (self.A, self.B, self.C)))
        self.tree = cKDTree(self.cent)
        e = np.concatenate([np.linalg.norm(self.B - self.A, axis=1), np.linalg.norm(self.C - self.B, axis=1),
                            np.linalg.norm(self.A - self.C, axis=1)])
        self.l_max = float(e.max())

    def query(self, pts):
        """per point: dist (unsigned), signed dist, face (lowest index among the exact float64 minima), closest,
        inside (closest point interior to the face), runner-up distance over the OTHER faces."""
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        N = pts.shape[0]
        out = {k: np.zeros(N) for k in ("dist", "signed", "second")}
        out["face"] = np.zeros(N, np.int64)
        out["closest"] = np.zeros((N, 3))
        out["inside"] = np.zeros(N, bool)
        _, near = self.tree.query(pts, k=1)
        for i in range(N):
            p = pts[i]
            f0 = int(near[i])
            d0 = point_triangles(p, self.A[f0], self.B[f0], self.C[f0])[0][0]
            cand = np.asarray(self.tree.query_ball_point(p, d0 + self.rmax + 1e-9 * (1 + d0)), np.int64)
            cand = np.union1d(cand, [f0])
            d, c, ins, side = point_triangles(p, self.A[cand], self.B[cand], self.C[cand])
            k = int(np.lexsort((cand, d))[0])
            out["dist"][i] = d[k]
            out["face"][i] = cand[k]
            out["closest"][i] = c[k]
            out["inside"][i] = ins[k]
            out["signed"][i] = -d[k] if side[k] < 0 else d[k]
            others = np.delete(d, k)
            out["second"][i] = others.min() if others.size else np.inf
        return out


def mesh_distance(gt_vs, gt_faces, org_vs, org_faces, out_vs, out_faces, eps=0.05, hole=None):
    """The metric of check/dist_check.py:35-67 in float64 (gt_faces: unused, kept for the call's symmetry)."""
    gt_vs = np.asarray(gt_vs, np.float64)
    q = SurfaceOracle(out_vs, out_faces).query(gt_vs)["signed"]
    q_org = None
    if hole is None:
        q_org = SurfaceOracle(org_vs, org_faces).query(gt_vs)["dist"]
        hole = q_org > eps
    diag = float(np.linalg.norm(gt_vs.max(0) - gt_vs.min(0)))
    hd_all = np.abs(q).sum() / len(q) / diag
    hd_hole = np.abs(q[hole]).sum() / hole.sum() / diag if hole.sum() else float("nan")
    return {"hd_all": hd_all, "hd_hole": hd_hole, "n_hole": int(hole.sum()), "diag": diag, "q": q, "hole": hole,
            "q_org": q_org}
