"""The sampling rule of semigcn_amd.evaluate (module docstring, "Sampling rule") restated in numpy and Python integers, and
the float64 restatement of the two reductions behind ``surface_distance``.

Every choice of the rule is integer arithmetic -- the weights are exact integer square roots, the face is a binary search
in an integer prefix sum, the barycentrics are 24-bit integers -- and the one floating-point expression (the point) is
plain float64 multiplies and adds of exactly representable products, rounded to float32 once.  So csrc/mesh_sample.hip
must equal this file bit for bit; tests/test_gpu_sampled_distance.py compares with ``torch.equal``."""
from __future__ import annotations

import math

import numpy as np

M32 = 0xFFFFFFFF
ONE = 1 << 24                         # the barycentrics are integers out of 2^24
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) on Python integers:
    counter = four 32-bit words, key = two; returns four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def isqrt_device(q: int) -> int:
    """The device's integer square root: a float64 estimate, then the two correcting loops -- whatever the estimate's
    rounding, the result is floor(sqrt(q))."""
    r = int(math.sqrt(float(q)))
    while r * r > q:
        r -= 1
    while (r + 1) * (r + 1) <= q:
        r += 1
    return r


def face_nn(vs, faces, face_mask=None):
    """nn [F] float64: the squared length of e1 x e2 per face, plain multiplies and adds in the rule's order; 0 where
    ``face_mask`` is 0.  ``ValueError`` for a vertex id outside [0, V) or a non-finite nn."""
    vs = np.asarray(vs, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= vs.shape[0]):
        raise ValueError(f"face refers to a vertex outside [0, {vs.shape[0]})")
    v = vs.astype(np.float64)
    A, B, C = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        e1, e2 = B - A, C - A
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        nn = (nx * nx + ny * ny) + nz * nz
    if not np.isfinite(nn).all():
        raise ValueError("a face has a non-finite squared normal")
    if face_mask is not None:
        nn = np.where(np.asarray(face_mask).reshape(-1) != 0, nn, 0.0)
    return nn


class SamplerOracle:
    """``w`` uint64 [F], ``cdf`` uint64 [F + 1], ``W``, ``s`` and ``n_zero_weight`` of the rule, and the draws."""

    def __init__(self, vs, faces, face_mask=None):
        self.vs = np.asarray(vs, np.float32).reshape(-1, 3)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        nn = face_nn(self.vs, self.faces, face_mask)
        F = self.faces.shape[0]
        m = float(nn.max()) if F else 0.0
        if m == 0.0:
            self.s = 0
            w = [0] * F
        else:
            _, e = math.frexp(m)                      # m = f 2^e, f in [0.5, 1)
            self.s = 62 - e
            q = np.floor(np.ldexp(nn, self.s))        # < 2^62: exact as a float64 and as a uint64
            w = [isqrt_device(int(x)) for x in q]
        self.w = np.asarray(w, np.uint64).reshape(F)
        cdf = [0]
        for x in w:
            cdf.append(cdf[-1] + x)
        self.W = cdf[-1]
        assert self.W < 1 << 63
        self.cdf = np.asarray(cdf, np.uint64)
        self.n_zero_weight = int(sum(1 for x in w if x == 0))

    def locate(self, t: int) -> int:
        """the f with cdf[f] <= t < cdf[f + 1]: upper bound minus one"""
        assert 0 <= t < self.W
        return int(np.searchsorted(self.cdf, np.uint64(t), side="right")) - 1

    def draw_one(self, seed: int, k: int):
        """(face, w0, a, b) of draw k"""
        x0, x1, x2, x3 = philox4x32_10((k & M32, (k >> 32) & M32, 0, 0), (seed & M32, (seed >> 32) & M32))
        r = x1 << 32 | x0
        t = (r * self.W) >> 64
        a, b = x2 >> 8, x3 >> 8
        if a + b > ONE:
            a, b = ONE - a, ONE - b
        return self.locate(t), ONE - a - b, a, b

    def draw(self, seed: int, offset: int, n: int, order: str = "face"):
        """dict of ``points`` float32 [n, 3], ``face`` int64 [n], ``bary`` int32 [n, 3] = (w0, a, b) and ``index`` int64
        [n] = k, in draw order or sorted by (face, k)."""
        if n > 0 and self.W == 0:
            raise ValueError("every face has weight 0")
        rows = [self.draw_one(seed, offset + i) + (offset + i,) for i in range(n)]
        if order == "face":
            rows.sort(key=lambda r: (r[0], r[4]))
        elif order != "draw":
            raise ValueError(order)
        face = np.asarray([r[0] for r in rows], np.int64).reshape(n)
        bary = np.asarray([r[1:4] for r in rows], np.int32).reshape(n, 3)
        index = np.asarray([r[4] for r in rows], np.int64).reshape(n)
        v = self.vs.astype(np.float64)
        fc = self.faces[face]
        A, B, C = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
        bw = bary.astype(np.float64)
        pts = ((bw[:, 0:1] * A + bw[:, 1:2] * B) + bw[:, 2:3] * C) * 2.0 ** -24
        return {"points": pts.astype(np.float32), "face": face, "bary": bary, "index": index}


def normals64(vs, faces):
    """(n [F, 3], nn [F]) in float64 from the float32 vertices"""
    v = np.asarray(vs, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n, (n * n).sum(1)


def normal_agreement(vs_a, faces_a, face_a, vs_b, faces_b, face_b):
    """(sum |cos|, count) over the pairs with face_a >= 0, face_b != 0x7fffffff and two non-zero normals; the sum by
    math.fsum."""
    na, nna = normals64(vs_a, faces_a)
    nb, nnb = normals64(vs_b, faces_b)
    face_a, face_b = np.asarray(face_a, np.int64), np.asarray(face_b, np.int64)
    ok = (face_a >= 0) & (face_b >= 0) & (face_b != 0x7FFFFFFF)
    fa, fb = face_a[ok], face_b[ok]
    ok2 = (nna[fa] > 0) & (nnb[fb] > 0)
    fa, fb = fa[ok2], fb[ok2]
    cos = (na[fa] * nb[fb]).sum(1) / np.sqrt(nna[fa] * nnb[fb])
    return math.fsum(np.abs(cos).tolist()), int(len(cos))


def distance_stats(dist, tau=None):
    """(max |d|, sum |d|, sum d^2, count |d| <= tau, skipped) over the rows that are not infinite; the sums by math.fsum
    on the float32 values widened to float64."""
    d = np.asarray(dist, np.float32)
    skip = np.isinf(d)
    a = np.abs(d[~skip]).astype(np.float64)
    within = int((np.abs(d[~skip]) <= np.float32(tau)).sum()) if tau is not None else 0
    return (float(a.max()) if a.size else 0.0, math.fsum(a.tolist()), math.fsum((a * a).tolist()), within, int(skip.sum()))
