"""The ray rule of ``semigcn_amd/render.py`` ("The rule") restated in numpy: every face against every ray, no tree.  Every
line below is an elementwise float64 operation on the widened float32 values, in the order the rule writes them (numpy fuses
nothing), so the device must equal it bit for bit.  Beside it: the camera rays, the shading in float64, the slab interval
of a box (for the tree-walk argument) and a predicate in Python ``Fraction``s, which is the truth on integer data."""
from fractions import Fraction

import numpy as np

NO_FACE = 0x7FFFFFFF
WIDE_UP, WIDE_DOWN = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
RAMP = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0]], np.float64)   # blue, cyan, green, yellow, red


def det3(u, v, w):
    return (u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2])) + u[2] * (v[0] * w[1] - v[1] * w[0])


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normals(vs, faces):
    """float64 n = (B - A) x (C - A), components as in normal_of; [3, F]."""
    v = np.asarray(vs, np.float32).astype(np.float64)
    A, B, C = (v[faces[:, k]].T for k in range(3))
    e1, e2 = B - A, C - A
    return np.stack([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])


def slab(lo, hi, o, d):
    """Clause 4 on boxes: lo / hi float32 [3, ...], o / d float64 [3, ...] (broadcast).  (ok, tn, tf)."""
    shape = np.broadcast(lo[0], o[0]).shape
    tn, tf, ok = np.full(shape, -np.inf), np.full(shape, np.inf), np.ones(shape, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            l, h = lo[k].astype(np.float64), hi[k].astype(np.float64)
            zero = np.broadcast_to(d[k] == 0.0, shape)
            inv = 1.0 / np.where(d[k] == 0.0, 1.0, d[k])
            t1, t2 = (l - o[k]) * inv, (h - o[k]) * inv
            ok &= np.where(zero, (l <= o[k]) & (o[k] <= h), True)
            tn = np.where(zero, tn, np.maximum(tn, np.minimum(t1, t2)))
            tf = np.where(zero, tf, np.minimum(tf, np.maximum(t1, t2)))
        tn = tn * np.where(tn > 0.0, WIDE_DOWN, WIDE_UP)
        tf = tf * np.where(tf > 0.0, WIDE_UP, WIDE_DOWN)
    return ok, tn, tf


def hits(vs, faces, origins, dirs, t_min=0.0, t_max=np.inf, pairwise=False):
    """(hit bool [N, F], t float64 [N, F], b1, b2 float64 [N, F]): clauses 1-5 for every (ray, face) pair; rays with a
    non-finite component or d = 0 hit nothing.  ``pairwise``: ``faces`` has one row per ray, and the results are [N, 1]."""
    vs32 = np.asarray(vs, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    v = vs32.astype(np.float64)
    face_axis = (slice(None), slice(None), None) if pairwise else (slice(None), None, slice(None))
    A, B, C = (v[faces[:, k]].T[face_axis] for k in range(3))                  # [3, 1, F]; pairwise [3, N, 1]
    o, d = o32.astype(np.float64).T[:, :, None], d32.astype(np.float64).T[:, :, None]   # [3, N, 1]
    n = normals(vs32, faces)
    usable = ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
              & ((n[0] != 0) | (n[1] != 0) | (n[2] != 0)))[face_axis[1:]]
    n = n[face_axis]
    good = (np.isfinite(o32).all(1) & np.isfinite(d32).all(1) & (d32 != 0).any(1))[:, None]
    with np.errstate(all="ignore"):
        a, b, c = A - o, B - o, C - o
        U, V, W = det3(d, b, c), det3(d, c, a), det3(d, a, b)
        Sb = (U + V) + W
        inside = (Sb != 0) & (((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0)))
        den = dot3(d, n)
        t = dot3(a, n) / den
        tri = vs32[faces]                                                       # [F, 3 corners, 3 axes]
        lo, hi = tri.min(1).T[face_axis], tri.max(1).T[face_axis]
        ok, tn, tf = slab(lo, hi, o, d)
        hit = good & usable & inside & (den != 0) & ok & (tn <= t) & (t <= tf) & (t_min <= t) & (t <= t_max)
        return hit, t, V / Sb, W / Sb


def _rows(hit, t, b1, b2):
    """The result rows of hit / t / b1 / b2 [N, F]: the smallest t, the lowest face id among equals."""
    N = hit.shape[0]
    tm = np.where(hit, t, np.inf).min(1) if hit.shape[1] else np.full(N, np.inf)
    pick = hit & (t == tm[:, None])
    any_hit = pick.any(1)
    f = np.where(any_hit, pick.argmax(1), 0)
    r = np.arange(N)
    t_out = np.where(any_hit, t[r, f], np.inf).astype(np.float32)
    face = np.where(any_hit, f, NO_FACE).astype(np.int32)
    bary = np.where(any_hit[:, None], np.stack([b1[r, f], b2[r, f]], 1), np.nan).astype(np.float32)
    return t_out, face, bary


def ray_cast(vs, faces, origins, dirs, t_min=0.0, t_max=np.inf, chunk=256):
    """(t float32 [N], face int32 [N], bary float32 [N, 2]) by brute force."""
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    out = [_rows(*hits(vs, faces, o[i:i + chunk], d[i:i + chunk], t_min, t_max)) for i in range(0, len(o), chunk)]
    if not out:
        return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32)
    return tuple(np.concatenate(x) for x in zip(*out))


def ray_cast_culled(vs, faces, origins, dirs, t_min=0.0, t_max=np.inf, chunk=32):
    """``ray_cast`` for many faces: still every face against every ray, but clause 4 first -- a face whose own box the ray
    misses is hit by nothing -- and clauses 1-3 and 5 only on the faces that some ray of the chunk has left."""
    vs32, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    tri = vs32[faces]
    lo, hi = tri.min(1).T[:, None, :], tri.max(1).T[:, None, :]
    out = []
    for i in range(0, len(o32), chunk):
        o, d = o32[i:i + chunk], d32[i:i + chunk]
        with np.errstate(all="ignore"):
            ok, tn, tf = slab(lo, hi, o.astype(np.float64).T[:, :, None], d.astype(np.float64).T[:, :, None])
        left = np.flatnonzero((ok & (tn <= tf)).any(0))
        t, face, bary = _rows(*hits(vs32, faces[left], o, d, t_min, t_max))
        face = np.where(face == NO_FACE, NO_FACE, left[np.minimum(face, max(len(left) - 1, 0))] if len(left) else NO_FACE)
        out.append((t, face.astype(np.int32), bary))
    return tuple(np.concatenate(x) for x in zip(*out))


def tree_cast(vs, faces, groups, tree, origins, dirs, t_min=0.0, t_max=np.inf):
    """The same rows by a walk over an arbitrary binary tree: ``groups`` a list of face-id arrays (the leaves), ``tree``
    nested pairs whose leaves are indices into ``groups``.  A node's box is the exact min / max of the vertices below it; a
    subtree is dropped iff its slab interval says so (tn > tf, tf < t_min, tn > min(t_max, best t)) -- one ray at a time,
    the children in the order given: the monotonicity argument, not a fast walk."""
    vs32, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)

    boxes = {}

    def prepare(node):
        ids = np.concatenate([prepare(c) for c in node]) if isinstance(node, tuple) else np.asarray(groups[node])
        p = vs32[faces[ids]].reshape(-1, 3)
        boxes[id(node)] = (p.min(0), p.max(0))
        return ids
    prepare(tree)
    T, Fc, Bc = [], [], []
    for i in range(len(o32)):
        o, d = o32[i].astype(np.float64), d32[i].astype(np.float64)
        best = [np.inf, NO_FACE, np.nan, np.nan]
        if np.isfinite(o32[i]).all() and np.isfinite(d32[i]).all() and (d32[i] != 0).any():
            def visit(node):
                lo, hi = boxes[id(node)]
                ok, tn, tf = slab(lo, hi, o, d)
                if not ok.all() or tn > tf or tf < t_min or tn > min(t_max, best[0]):
                    return
                if isinstance(node, tuple):
                    for c in node:
                        visit(c)
                    return
                ids = groups[node]
                hit, t, b1, b2 = hits(vs32, faces[ids], o32[i:i + 1], d32[i:i + 1], t_min, t_max)
                for k in np.nonzero(hit[0])[0]:
                    if t[0, k] < best[0] or (t[0, k] == best[0] and ids[k] < best[1]):
                        best[:] = [t[0, k], int(ids[k]), b1[0, k], b2[0, k]]
            visit(tree)
        T.append(best[0] if best[1] != NO_FACE else np.inf)
        Fc.append(best[1])
        Bc.append(best[2:])
    return np.asarray(T, np.float64).astype(np.float32), np.asarray(Fc, np.int32), np.asarray(Bc, np.float64).reshape(-1, 2).astype(np.float32)


# ---- integer data: the truth in Fractions ------------------------------------------------------------------------------

def _idet3(u, v, w):
    return u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def ray_cast_exact(vs, faces, origins, dirs, t_min=0, t_max=None):
    """The rows for INTEGER vs / origins / dirs in exact arithmetic: clauses 1, 2, 3 and 5 (clause 4 holds for every exact
    hit: the point lies in the face, so in its box).  t and bary are rounded to float64 and then to float32, as the rule's
    one division and its store do."""
    vs = [[int(x) for x in p] for p in np.asarray(vs).tolist()]
    faces = [[int(x) for x in f] for f in np.asarray(faces).tolist()]
    T, Fc, Bc = [], [], []
    for o, d in zip(np.asarray(origins).tolist(), np.asarray(dirs).tolist()):
        o, d = [int(x) for x in o], [int(x) for x in d]
        best = None
        for f, (ia, ib, ic) in enumerate(faces):
            if not any(d) or len({ia, ib, ic}) < 3:
                continue
            A, B, C = vs[ia], vs[ib], vs[ic]
            e1, e2 = [B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            if not any(n):
                continue
            a, b, c = ([P[k] - o[k] for k in range(3)] for P in (A, B, C))
            U, V, W = _idet3(d, b, c), _idet3(d, c, a), _idet3(d, a, b)
            Sb = U + V + W
            if Sb == 0 or not (min(U, V, W) >= 0 or max(U, V, W) <= 0):
                continue
            den = sum(d[k] * n[k] for k in range(3))
            if den == 0:
                continue
            t = Fraction(sum(a[k] * n[k] for k in range(3)), den)
            if t < t_min or (t_max is not None and t > t_max):
                continue
            if best is None or t < best[0]:
                best = (t, f, Fraction(V, Sb), Fraction(W, Sb))
        T.append(np.inf if best is None else float(best[0]))
        Fc.append(NO_FACE if best is None else best[1])
        Bc.append([np.nan, np.nan] if best is None else [float(best[2]), float(best[3])])
    return np.asarray(T, np.float64).astype(np.float32), np.asarray(Fc, np.int32), np.asarray(Bc, np.float64).reshape(-1, 2).astype(np.float32)


# ---- the camera and the shading ---------------------------------------------------------------------------------------

def camera_rays(cam, ortho, width, height):
    """(origins, dirs) float32 [H * W, 3] of the primary rays, pixel (x, y) at row y * width + x; ``cam`` = the 14 float64
    values eye, right, up, forward, tx, ty."""
    cam = np.asarray(cam, np.float64)
    e, r, u, w, tx, ty = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
    y, x = (g.reshape(-1).astype(np.float64) for g in np.meshgrid(np.arange(height), np.arange(width), indexing="ij"))
    sx = ((2.0 * (x + 0.5)) / float(width) - 1.0) * tx
    sy = (1.0 - (2.0 * (y + 0.5)) / float(height)) * ty
    off = np.stack([(b[k] + sx * r[k]) + sy * u[k] for k in range(3) for b in [e if ortho else w]], 1)
    fixed = np.broadcast_to((w if ortho else e), off.shape)
    o, d = (off, fixed) if ortho else (fixed, off)
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d.astype(np.float32))


def ramp(x):
    """colour levels float64 [..., 3] in [0, 255] of x in [0, 1]: five stops, piecewise linear."""
    u = x * 4.0
    k = np.minimum(u.astype(np.int64), 3)
    f = (u - k)[..., None]
    return 255.0 * (RAMP[k] + f * (RAMP[k + 1] - RAMP[k]))


def shade(vs, faces, face, bary, dirs, *, color=(255, 165, 0), face_colors=None, scalars=None, vmin=0.0, vmax=1.0,
          background=(255, 255, 255), ambient=0.25):
    """rgb uint8 [n, 3] and the float64 values before the floor [n, 3] (NaN on the background)."""
    vs32, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    face = np.asarray(face).reshape(-1)
    hit = face != NO_FACE
    f = np.where(hit, face, 0)
    n = normals(vs32, faces)[:, f]
    d = np.asarray(dirs, np.float32).astype(np.float64).T
    with np.errstate(all="ignore"):
        len2 = dot3(d, d) * dot3(n, n)
        inten = np.where(len2 > 0, ambient + ((1.0 - ambient) * np.abs(dot3(d, n))) / np.sqrt(len2), ambient)
        if face_colors is not None:
            level = np.asarray(face_colors, np.uint8)[f].astype(np.float64)
        elif scalars is not None:
            s = np.asarray(scalars, np.float32).astype(np.float64)
            b1, b2 = (np.asarray(bary, np.float32).astype(np.float64).reshape(-1, 2)[:, k] for k in range(2))
            ids = faces[f]
            sv = (((1.0 - b1) - b2) * s[ids[:, 0]] + b1 * s[ids[:, 1]]) + b2 * s[ids[:, 2]]
            x = (sv - vmin) / (vmax - vmin) if vmax > vmin else np.zeros_like(sv)
            x = np.where(x > 0.0, np.where(x > 1.0, 1.0, x), 0.0)
            level = ramp(x)
        else:
            level = np.broadcast_to(np.asarray(color, np.float64), (len(face), 3))
        raw = level * inten[:, None] + 0.5
    raw = np.where(hit[:, None], raw, np.nan)
    rgb = np.where(hit[:, None], np.clip(np.floor(np.nan_to_num(raw)), 0, 255), np.asarray(background, np.float64)).astype(np.uint8)
    return rgb, raw


def ssaa_average(img, s):
    """uint8 [s H, s W, 3] -> uint8 [H, W, 3]: (sum + s*s // 2) // (s*s) in integers."""
    H, W = img.shape[0] // s, img.shape[1] // s
    total = img.astype(np.int64).reshape(H, s, W, s, 3).sum((1, 3))
    return ((total + s * s // 2) // (s * s)).astype(np.uint8)
