"""The vertex update of semigcn_amd/denoise.py ("The rule") restated in numpy, in explicit float32 operation order: what
csrc/mesh_denoise.hip must equal bit for bit.  Every product, sum and quotient below is one numpy float32 operation on
arrays, so each is rounded once and nothing is fused.  The loop runs over the valence rank r (the r-th incident face of
every vertex that has one), not over the vertices, so that 300 K vertices take seconds.

Also here: the face normals, the mean angle between two normal fields and a dense uniform Laplacian step, for the premises
of tests/test_denoise_oracle.py."""
import numpy as np

F32 = np.float32


def face_lists(faces, V):
    """(rowptr int64 [V + 1], vf int64 [3 F]): the faces that name each vertex, ascending inside a row."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    corners = faces.reshape(-1)
    order = np.argsort(corners, kind="stable")            # corners are face-major: a stable sort keeps ascending faces
    vf = order // 3
    rowptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(corners, minlength=V), out=rowptr[1:])
    return rowptr, vf


def centroids(p, faces):
    s = (p[faces[:, 0]] + p[faces[:, 1]]) + p[faces[:, 2]]
    return s / F32(3.0)


def step(p, faces, normals, rowptr, vf, movable=None):
    """One step from float32 [V, 3]; returns a new array."""
    V = p.shape[0]
    k = rowptr[1:] - rowptr[:-1]
    c = centroids(p, faces)
    s = np.zeros((V, 3), F32)
    for r in range(int(k.max()) if V else 0):
        sel = np.nonzero(k > r)[0]
        f = vf[rowptr[sel] + r]
        n = normals[f]
        d = c[f] - p[sel]
        t = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        s[sel] = s[sel] + t[:, None] * n
    move = k > 0
    if movable is not None:
        move &= np.asarray(movable).reshape(-1) != 0
    out = p.copy()
    with np.errstate(invalid="ignore"):
        out[move] = p[move] + s[move] / k[move].astype(F32)[:, None]
    return out


def update_vertices(vs, faces, normals, steps=10, movable=None):
    """``steps`` steps of the rule; float32 [V, 3]."""
    p = np.ascontiguousarray(vs, F32).reshape(-1, 3).copy()
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    assert normals.shape[0] == faces.shape[0]
    if faces.shape[0] == 0:
        return p
    rowptr, vf = face_lists(faces, p.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(int(steps)):
            p = step(p, faces, normals, rowptr, vf, movable)
    return p


def face_normals(vs, faces):
    """Unit face normals in float64 (zero for a face without area)."""
    vs = np.asarray(vs, np.float64)
    n = np.cross(vs[faces[:, 1]] - vs[faces[:, 0]], vs[faces[:, 2]] - vs[faces[:, 0]])
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def mean_normal_angle(vs, faces, clean_vs):
    """Mean angle in degrees between the face normals of ``vs`` and those of ``clean_vs`` over the same faces."""
    d = np.sum(face_normals(vs, faces) * face_normals(clean_vs, faces), axis=1)
    return float(np.degrees(np.arccos(np.clip(d, -1.0, 1.0))).mean())


def unique_edges(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def laplacian_step(vs, faces):
    """One step of uniform Laplacian smoothing on a closed mesh: p_i <- (p_i + 2 sum_j p_j) / (1 + 2 d_i), the rule of
    prepare.laplacian_smooth where every edge has two faces."""
    vs = np.asarray(vs, np.float64)
    e = unique_edges(faces)
    acc, deg = vs.copy(), np.ones(len(vs))
    for a, b in ((0, 1), (1, 0)):
        np.add.at(acc, e[:, a], 2.0 * vs[e[:, b]])
        np.add.at(deg, e[:, a], 2.0)
    return (acc / deg[:, None]).astype(F32)


def noisy_box(n=12, sigma=0.12, seed=7):
    """(clean float32 [V, 3], noisy float32 [V, 3], faces): ``synth.box_mesh(n)`` scaled to mean edge length 1, and the same
    with Gaussian noise of ``sigma`` from ``default_rng(seed)``."""
    from semigcn_amd import synth
    vs, faces = synth.box_mesh(n)
    e = unique_edges(faces)
    vs64 = vs.astype(np.float64)
    vs64 = vs64 / np.linalg.norm(vs64[e[:, 0]] - vs64[e[:, 1]], axis=1).mean()
    noisy = vs64 + np.random.default_rng(seed).normal(0.0, sigma, vs64.shape)
    return vs64.astype(F32), noisy.astype(F32), faces
