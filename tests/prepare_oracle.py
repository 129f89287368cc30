"""float64 numpy restatement of semigcn_amd.prepare: the smoothing rule, the mean edge length and the scan mask.

The smoothing works per face-edge incidence, the way vcglib's VertexCoordLaplacian walks a mesh, and never forms the
weights w_ij of the rule in semigcn_amd/prepare.py::laplacian_smooth -- it is an independent derivation of them:

  1. every face-edge (a, b) that is NOT a border edge adds p_b to a's sum and p_a to b's, and 1 to both counts
     (an edge shared by k faces is met k times: the weight k_ij);
  2. the two ends of every border face-edge have their sum and count reset to zero;
  3. every border face-edge then adds p_b to a and p_a to b, and 1 to both counts;
  4. p_i <- (p_i + sum_i) / (1 + count_i) where count_i > 0 and the vertex may move.

A border edge is an undirected edge that exactly one face-edge uses.  The mask uses the brute-force closest point of
tests/mesh_distance_oracle.py."""
from __future__ import annotations

import numpy as np

from mesh_distance_oracle import SurfaceOracle


def _face_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = f.reshape(-1)
    b = f[:, [1, 2, 0]].reshape(-1)
    return a, b


def _border_flags(a, b, V):
    key = np.minimum(a, b) * np.int64(max(V, 1)) + np.maximum(a, b)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] == 1


def smooth_step(p, faces, movable=None):
    p = np.asarray(p, np.float64)
    V = p.shape[0]
    a, b = _face_edges(faces)
    border = _border_flags(a, b, V)
    S, C = np.zeros((V, 3)), np.zeros(V)

    def accumulate(sel):
        np.add.at(S, a[sel], p[b[sel]])
        np.add.at(S, b[sel], p[a[sel]])
        np.add.at(C, a[sel], 1.0)
        np.add.at(C, b[sel], 1.0)
    accumulate(~border)
    ends = np.union1d(a[border], b[border])
    S[ends] = 0.0
    C[ends] = 0.0
    accumulate(border)
    move = C > 0
    if movable is not None:
        move &= np.asarray(movable, bool).reshape(-1)
    out = p.copy()
    out[move] = (p[move] + S[move]) / (1.0 + C[move])[:, None]
    return out


def smooth(vs, faces, steps, movable=None):
    p = np.asarray(vs, np.float64).copy()
    for _ in range(int(steps)):
        p = smooth_step(p, faces, movable)
    return p


def neighbour_lists(faces, V):
    """(longest neighbour list, per-vertex sum of the step's weights as the incidence walk counts them)."""
    a, b = _face_edges(faces)
    if a.size == 0:
        return 0, np.zeros(V)
    pairs = np.unique(np.concatenate([a * np.int64(V) + b, b * np.int64(V) + a]))
    d_max = int(np.bincount(pairs // V, minlength=V).max())
    border = _border_flags(a, b, V)
    C = np.zeros(V)
    np.add.at(C, a[~border], 1.0)
    np.add.at(C, b[~border], 1.0)
    ends = np.union1d(a[border], b[border])
    C[ends] = 0.0
    np.add.at(C, a[border], 1.0)
    np.add.at(C, b[border], 1.0)
    return d_max, C


def unique_edges(faces, V):
    a, b = _face_edges(faces)
    key = np.unique(np.minimum(a, b) * np.int64(max(V, 1)) + np.maximum(a, b))
    return np.stack([key // max(V, 1), key % max(V, 1)], 1)


def mean_edge_length(vs, edges):
    vs = np.asarray(vs, np.float64)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(np.linalg.norm(vs[e[:, 0]] - vs[e[:, 1]], axis=1).sum()) / np.float64(e.shape[0])


def scan_distances(initial_vs, original_vs, original_faces):
    return SurfaceOracle(original_vs, original_faces).query(initial_vs)["dist"]


def scan_mask(initial_vs, original_vs, original_faces, eps=0.2):
    return scan_distances(initial_vs, original_vs, original_faces) < eps
