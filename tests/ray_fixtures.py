"""Meshes and rays the ray tests share, each built (and its reference computed) once per process."""
import functools
import struct
import zlib

import numpy as np

import ray_oracle as R
from semigcn_amd import synth


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vs float32 [V, 3], faces int64 [F, 3]) of "sphere" (octahedron_sphere(3)) or "torus" (torus_mesh(20, 12))."""
    m = synth.octahedron_sphere(3) if name == "sphere" else synth.torus_mesh(20, 12)
    return np.ascontiguousarray(m.vs.astype(np.float32)), np.ascontiguousarray(m.faces.astype(np.int64))


def edges_of(faces):
    return np.unique(np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1), axis=0)


@functools.lru_cache(maxsize=None)
def feature_targets(name):
    """(vertices, edge midpoints, centroids) of a mesh as float32 points, and for each the list of face-id arrays that share
    the feature."""
    vs, faces = mesh(name)
    v64 = vs.astype(np.float64)
    e = edges_of(faces)
    mid = (0.5 * (v64[e[:, 0]] + v64[e[:, 1]])).astype(np.float32)
    cen = v64[faces].mean(1).astype(np.float32)
    at_v = [np.nonzero((faces == i).any(1))[0] for i in range(len(vs))]
    at_e = [np.nonzero((faces == a).any(1) & (faces == b).any(1))[0] for a, b in e]
    at_c = [np.array([i]) for i in range(len(faces))]
    return (vs, mid, cen), (at_v, at_e, at_c)


def feature_rays(name, inside):
    """Rays through every vertex, edge midpoint and centroid: from the centre of the sphere (0, 0, 0) when ``inside``, else
    from three times as far out towards it.  Only the sphere has a centre that sees every feature first."""
    (v, m, c), (av, ae, ac) = feature_targets(name)
    tg = np.concatenate([v, m, c])
    if inside:
        return np.zeros_like(tg), tg, av + ae + ac
    return (3.0 * tg).astype(np.float32), -tg, av + ae + ac


def random_lines(name, n=600, seed=1):
    """``n`` seeded lines through the mesh's box; the first sixth has one zero direction component, the next twelfth two."""
    vs, _ = mesh(name)
    rng = np.random.default_rng(seed)
    c = vs.mean(0)
    r = np.abs(vs - c).max()
    o = (c + rng.uniform(-1, 1, (n, 3)) * r).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:n // 6, 0] = 0
    d[n // 6:n // 4, 1] = 0
    d[n // 6:n // 4, 2] = 0
    return o, d


@functools.lru_cache(maxsize=None)
def int_box():
    """The box [0, 8]^3 with 768 faces on integer coordinates, integer rays, and their rows in exact arithmetic."""
    vs, faces = synth.box_mesh(8)
    vs = np.rint(vs * 8).astype(np.float32)
    o, d = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for j in range(0, 9, 2):
            for k, step in ((0, 1), (8, 1), (3, 1), (j, 2)):     # in the planes of two sides, inside, t = 1.5
                p, q = np.zeros(3, int), np.zeros(3, int)
                p[axis], p[u], p[v] = -3, j, k
                q[axis] = step
                o.append(p)
                d.append(q)
                o.append(np.where(np.arange(3) == axis, 11, p))    # and from the other end
                d.append(-q)
    for p, q in (((-2, -2, 0), (1, 1, 0)), ((-2, -2, 4), (1, 1, 0)), ((-1, -1, -1), (1, 1, 1)), ((9, 9, 9), (-1, -1, -1)),
                 ((-2, 3, 0), (2, 1, 0)), ((-4, 0, 8), (2, 1, 0)), ((10, -2, 5), (-1, 1, 0)), ((4, 4, 4), (1, 2, 3)),
                 ((4, 4, 4), (0, 0, -1)), ((4, 4, 4), (-3, 0, 1)), ((-1, 4, 4), (-1, 0, 0)), ((0, 0, -5), (0, 0, 2)),
                 ((8, 8, -3), (0, 0, 2)), ((20, 20, 20), (1, 0, 0)), ((-2, 4, 0), (2, 0, 1)), ((3, -6, 3), (1, 4, 1))):
        o.append(np.array(p))
        d.append(np.array(q))
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    return vs, faces, o, d, R.ray_cast_exact(vs, faces, o, d)


def one_face_copies(n):
    """``n`` copies of one face over three vertices: equal keys, a deep tree, the lowest id wins."""
    vs = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
    return vs, np.tile(np.array([[0, 1, 2]], np.int64), (n, 1))


def needles():
    """Needles of aspect 1e5 at coordinates near 1e3: a fan of 24 thin faces in the plane z = 1000 + a small tilt."""
    rng = np.random.default_rng(5)
    k = 24
    a = np.stack([1000 + np.arange(k) * 1e-4, np.full(k, 1000.0), 1000 + rng.uniform(-1e-3, 1e-3, k)], 1)
    b = a + np.array([1e-4, 0, 0])
    c = a + np.array([5e-5, 10.0, 0.01])
    vs = np.concatenate([a, b, c]).astype(np.float32)
    faces = np.stack([np.arange(k), k + np.arange(k), 2 * k + np.arange(k)], 1).astype(np.int64)
    t = rng.uniform(0.05, 0.95, (200, 1))
    f = rng.integers(0, k, 200)
    target = (vs[faces[f, 0]] * (1 - t) * 0.5 + vs[faces[f, 1]] * (1 - t) * 0.5 + vs[faces[f, 2]] * t).astype(np.float32)
    o = (target + np.array([0.3, -0.2, 5.0])).astype(np.float32)
    return vs, faces, o, (target - o).astype(np.float32)


def bits(x):
    """an array's bytes, for equality that tells -0 from +0 and one NaN from another"""
    return np.ascontiguousarray(x).view(np.uint8)


def assert_rows_equal(got, want, what="", zero_sign=True):
    """(t, face, bary) rows equal bit for bit.  ``zero_sign=False``: -0 equals +0 -- for a reference in exact arithmetic,
    which has no signed zero (the rule's 0 / -Sb is -0)."""
    for g, w, n in zip(got, want, ("t", "face", "bary")):
        g, w = np.asarray(g), np.asarray(w)
        if not zero_sign and n != "face":
            g, w = g + np.float32(0), w + np.float32(0)         # -0 + 0 = +0
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, w.dtype, g.shape, w.shape)
        if n == "bary":                                     # a NaN row is a NaN row
            nan_g, nan_w = np.isnan(g), np.isnan(w)
            assert np.array_equal(nan_g, nan_w), (what, n)
            g, w = np.where(nan_g, 0, g), np.where(nan_w, 0, w)
        bad = np.nonzero((bits(g).reshape(len(g), -1) != bits(w).reshape(len(w), -1)).any(1))[0] if len(g) else []
        assert len(bad) == 0, (what, n, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def read_png(path):
    """A minimal reader for what write_png / write_apng write: 8-bit truecolour, filter 0 rows.  uint8 [N, H, W, 3] and the
    delays in ms."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    frames, delays, seq = [], [], 0
    for kind, body in chunks[1:-1]:
        if kind == b"acTL":
            n_frames, plays = struct.unpack(">II", body)
            assert plays == 0
        elif kind == b"fcTL":
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (s, w, h, x, y, dispose, blend) == (seq, W, H, 0, 0, 0, 0)
            delays.append(1000 * num // den)
            seq += 1
        elif kind in (b"IDAT", b"fdAT"):
            if kind == b"fdAT":
                assert struct.unpack(">I", body[:4])[0] == seq
                seq, body = seq + 1, body[4:]
            rows = np.frombuffer(zlib.decompress(body), np.uint8).reshape(H, 1 + 3 * W)
            assert (rows[:, 0] == 0).all()
            frames.append(rows[:, 1:].reshape(H, W, 3))
    if delays:
        assert n_frames == len(frames) == len(delays)
    return np.stack(frames), delays
