"""Plain numpy restatement of semigcn_amd.components: a serial union-find over the links of the module docstring, the
canonical numbering, the tie rule, ``keep`` / ``min_faces`` and the stable compaction -- no sort, no scan, no atomics.
Also the meshes the tests share."""
from __future__ import annotations

import numpy as np


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def degenerate(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])


def face_components(faces, num_vertices, connectivity="edge"):
    """(labels int64 [F] with -1 = degenerate, face_count int64 [K], largest, n_degenerate)."""
    if connectivity not in ("edge", "vertex"):
        raise ValueError(connectivity)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = f.shape[0], int(num_vertices)
    if F and (f.min() < 0 or f.max() >= V):
        raise ValueError("vertex index out of range")
    bad = degenerate(f)
    faces_l = f.tolist()
    root_of_face = [-1] * F
    if connectivity == "edge":
        parent = list(range(F))
        first = {}                                    # undirected edge -> the first face seen on it
        for i, (a, b, c) in enumerate(faces_l):
            if bad[i]:
                continue
            for u, v in ((a, b), (b, c), (c, a)):
                e = (u, v) if u < v else (v, u)
                if e in first:
                    _union(parent, first[e], i)
                else:
                    first[e] = i
        for i in range(F):
            if not bad[i]:
                root_of_face[i] = _find(parent, i)
    else:
        parent = list(range(V))
        for i, (a, b, c) in enumerate(faces_l):
            if not bad[i]:
                _union(parent, a, b)
                _union(parent, b, c)
        for i, (a, _b, _c) in enumerate(faces_l):
            if not bad[i]:
                root_of_face[i] = _find(parent, a)
    labels = np.full(F, -1, np.int64)
    number = {}                                       # root -> id, in order of first (= smallest) face
    for i in range(F):
        if not bad[i]:
            labels[i] = number.setdefault(root_of_face[i], len(number))
    K = len(number)
    count = np.bincount(labels[labels >= 0], minlength=K).astype(np.int64)
    largest = int(np.argmax(count)) if K else -1      # argmax returns the first of equals: the lower id
    return labels, count, largest, int(bad.sum())


def keep_mask(keep, count, largest, min_faces=None):
    K = count.shape[0]
    if isinstance(keep, str):
        mask = np.zeros(K, bool)
        if keep == "all":
            mask[:] = True
        elif keep == "largest":
            if largest >= 0:
                mask[largest] = True
        else:
            raise ValueError(keep)
    else:
        mask = np.asarray(keep).reshape(-1) != 0
        assert mask.shape[0] == K
    if min_faces is not None:
        mask = mask & (count >= min_faces)
    return mask


def keep_components(vs, faces, keep="largest", min_faces=None, connectivity="edge"):
    """(new_vs float32 [V', 3], new_faces int64 [F', 3], vertex_ids int64 [V'], face_ids int64 [F'], kept bool [K])."""
    vs = np.asarray(vs, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    labels, count, largest, _ = face_components(f, vs.shape[0], connectivity)
    mask = keep_mask(keep, count, largest, min_faces)
    new_vs, new_faces, vertex_ids, face_ids = [], [], [], []
    used = set()
    for i in range(f.shape[0]):
        if labels[i] >= 0 and mask[labels[i]]:
            used.update(f[i].tolist())
    new_id = {}
    for v in range(vs.shape[0]):
        if v in used:
            new_id[v] = len(vertex_ids)
            vertex_ids.append(v)
            new_vs.append(vs[v])
    for i in range(f.shape[0]):
        if labels[i] >= 0 and mask[labels[i]]:
            face_ids.append(i)
            new_faces.append([new_id[v] for v in f[i].tolist()])
    return (np.asarray(new_vs, np.float32).reshape(-1, 3), np.asarray(new_faces, np.int64).reshape(-1, 3),
            np.asarray(vertex_ids, np.int64), np.asarray(face_ids, np.int64), mask)


# ---- meshes ------------------------------------------------------------------------------------------------------------
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64)
OCT_VS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCT = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


def two_tetrahedra_sharing_a_vertex():
    """Vertex 3 is the apex of both: (V = 7, faces [8, 3])."""
    other = np.array([3, 4, 5, 6])[TET]
    return 7, np.concatenate([TET, other])


def fan(n):
    """n faces around the edge (0, 1): (V = n + 2, faces [n, 3]); every second face is turned round."""
    f = np.array([[0, 1, 2 + i] if i % 2 == 0 else [1, 0, 2 + i] for i in range(n)], np.int64)
    return n + 2, f


def strip(n_quads):
    """Open 1 x n strip: vertices 2 i (bottom) and 2 i + 1 (top), faces (2 i, 2 i + 2, 2 i + 1), (2 i + 1, 2 i + 2, 2 i + 3):
    the face graph is a path."""
    i = np.arange(n_quads, dtype=np.int64)
    f = np.stack([np.stack([2 * i, 2 * i + 2, 2 * i + 1], 1), np.stack([2 * i + 1, 2 * i + 2, 2 * i + 3], 1)], 1)
    return 2 * (n_quads + 1), f.reshape(-1, 3)


def octahedra(n, interleave=True):
    """n octahedra on disjoint vertex sets: (vs float32 [6 n, 3], faces [8 n, 3]); interleaved: face j of octahedron i is
    face j * n + i, so that no component's faces are contiguous."""
    vs = (OCT_VS[None] * 0.25 + np.stack([np.arange(n), np.zeros(n), np.zeros(n)], 1)[:, None, :]).reshape(-1, 3)
    f = 6 * np.arange(n, dtype=np.int64)[:, None, None] + OCT[None]            # [n, 8, 3]
    f = f.transpose(1, 0, 2) if interleave else f
    return vs.astype(np.float32), np.ascontiguousarray(f.reshape(-1, 3))
