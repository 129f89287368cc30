"""The premises of tests/sample_oracle.py, the numpy restatement of the sampling rule of semigcn_amd.evaluate: known
answers of the generator and of the rule on a two-face mesh, the weight edge cases, the fold, and that the new C entry
points refuse bad arguments before any device is touched.  No GPU."""
import ctypes
import math

import numpy as np

import sample_oracle as SO
from semigcn_amd import capi

TWO_VS = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [0, 0, 1], [1, 0, 1], [0, 2, 1]], np.float32)
TWO_FACES = np.array([[0, 1, 2], [3, 4, 5]], np.int64)


def test_philox_known_answers():
    """Philox4x32-10: the three known-answer vectors of the Random123 distribution (counter / key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join("%08x" % x for x in SO.philox4x32_10(counter, key)) == want


def test_two_face_mesh_known_answers():
    o = SO.SamplerOracle(TWO_VS, TWO_FACES)
    assert o.w.tolist() == [1610612736, 536870912] and o.W == 1 << 31 and o.cdf.tolist() == [0, 1610612736, 1 << 31]
    assert o.n_zero_weight == 0
    assert [o.draw_one(7, k) for k in range(3)] == [(1, 13424538, 1915578, 1437100), (1, 2175213, 13894913, 707090),
                                                    (0, 11011484, 3227012, 2538720)]
    d = o.draw(7, 0, 3, order="draw")
    assert d["points"][0].astype(np.float64).tolist() == [0.11417734622955322, 0.17131567001342773, 1.0]
    assert d["index"].tolist() == [0, 1, 2] and d["face"].tolist() == [1, 1, 0]
    f = o.draw(7, 0, 3, order="face")
    assert f["index"].tolist() == [2, 0, 1] and f["face"].tolist() == [0, 1, 1]           # sorted by (face, k)
    assert np.array_equal(f["points"], d["points"][[2, 0, 1]]) and np.array_equal(f["bary"], d["bary"][[2, 0, 1]])
    # the carry into the counter's high word, and the key's high word
    seed, offset = (5 << 32) | 9, (1 << 32) - 2
    assert [o.draw_one(seed, offset + i) for i in range(4)] == [(0, 1953445, 13098944, 1724827), (0, 8595197, 2118188, 6063831),
                                                                (1, 8573711, 1497227, 6706278), (0, 718945, 6244660, 9813611)]
    assert o.draw(seed, offset, 4, order="draw")["index"].tolist() == [offset + i for i in range(4)]


def test_area_proportionality():
    """Face 0 has 3/4 of the area: of 4096 draws 3072 are expected on it, and six binomial standard deviations
    (sqrt(4096 * 3/4 * 1/4) = 27.7) are 166."""
    o = SO.SamplerOracle(TWO_VS, TWO_FACES)
    count = sum(o.draw_one(7, k)[0] == 0 for k in range(4096))
    assert count == 3023
    assert abs(count - 3072) <= 166


def test_isqrt_edges():
    for r in (1 << 30, (1 << 30) - 1, (1 << 30) + 1, (1 << 31) - 1, 1, 2, 3037000499):
        assert SO.isqrt_device(r * r - 1) == r - 1
        assert SO.isqrt_device(r * r) == r
        assert SO.isqrt_device(r * r + 2 * r) == r
        for q in (r * r - 1, r * r, r * r + 2 * r):
            assert SO.isqrt_device(q) == math.isqrt(q)
    assert SO.isqrt_device(0) == 0


def test_weight_edge_cases():
    t = 2.0 ** -33
    vs = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0],
                   [0, 0, 0], [t, 0, 0], [0, t, 0]], np.float32)
    unit = math.isqrt(1 << 61)                   # nn = 1 = 0.5 * 2^1: s = 61, q = 2^61
    # a unit face beside one with edge 2^-33: the ratio of the areas is 2^-66, far below 2^-31
    o = SO.SamplerOracle(vs, [[0, 1, 2], [6, 7, 8]])
    assert o.s == 61 and o.w.tolist() == [unit, 0] and o.n_zero_weight == 1 and o.W == unit
    # a masked face has weight 0, whatever its area
    o = SO.SamplerOracle(vs, [[0, 1, 2], [0, 2, 1], [6, 7, 8]], face_mask=[0, 1, 1])
    assert o.w.tolist() == [0, unit, 0] and o.n_zero_weight == 2
    assert all(o.draw_one(3, k)[0] == 1 for k in range(64))
    # m == 0: every weight is 0 and there is nothing to draw from
    for faces, mask in (([[0, 0, 1], [2, 2, 2]], None), ([[0, 1, 2]], [0])):
        o = SO.SamplerOracle(vs, faces, face_mask=mask)
        assert o.W == 0 and o.s == 0 and not o.w.any() and o.n_zero_weight == len(faces)
        try:
            o.draw(0, 0, 1)
        except ValueError:
            pass
        else:
            raise AssertionError("a draw from a surface of weight 0 must be refused")
        assert o.draw(0, 0, 0)["points"].shape == (0, 3)
    # a bad index and a non-finite vertex are errors
    for bad_vs, bad_faces in ((vs, [[0, 1, 9]]), (vs, [[0, 1, -1]]), (np.where(np.arange(27).reshape(9, 3) == 4, np.nan, vs), [[0, 1, 2]]),
                              (np.where(np.arange(27).reshape(9, 3) == 4, np.inf, vs), [[0, 1, 2]])):
        try:
            SO.SamplerOracle(bad_vs, bad_faces)
        except ValueError:
            continue
        raise AssertionError("must be refused")


def test_fold_keeps_the_barycentrics_in_the_triangle():
    o = SO.SamplerOracle(TWO_VS, TWO_FACES)
    folded = 0
    for k in range(2000):
        x = SO.philox4x32_10((k, 0, 0, 0), (11, 0))
        _, w0, a, b = o.draw_one(11, k)
        folded += (x[2] >> 8) + (x[3] >> 8) > SO.ONE
        assert w0 + a + b == SO.ONE and min(w0, a, b) >= 0
    assert 800 < folded < 1200          # both branches are taken


def test_points_lie_in_their_faces():
    """Every point of a 200-draw run lies in the plane of its face and inside it, to the float32 rounding of the point."""
    rng = np.random.default_rng(5)
    vs = rng.normal(0, 3, (40, 3)).astype(np.float32)
    faces = rng.integers(0, 40, (60, 3))
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]
    o = SO.SamplerOracle(vs, faces)
    d = o.draw(21, 0, 200)
    assert np.all(np.diff(d["face"]) >= 0) and len(set(d["index"].tolist())) == 200
    v = vs.astype(np.float64)
    A, B, C = (v[faces[d["face"], k]] for k in range(3))
    p = d["points"].astype(np.float64)
    ulp = np.abs(np.stack([A, B, C])).max() * 2.0 ** -23            # float32 rounding of a coordinate of the point
    n = np.cross(B - A, C - A)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(((p - A) * n).sum(1)).max() <= 2 * ulp
    # barycentric coordinates of the rounded point, uv = T^+ (p - A): a displacement of the point by at most sqrt(3) ulp
    # moves them by at most that over the smallest singular value of T = [B - A, C - A]
    T = np.stack([B - A, C - A], 2)
    uv = np.stack([np.linalg.lstsq(T[i], p[i] - A[i], rcond=None)[0] for i in range(len(p))])
    want = d["bary"][:, 1:].astype(np.float64) / SO.ONE
    tol = math.sqrt(3.0) * ulp / np.linalg.svd(T, compute_uv=False).min(1)
    assert (np.abs(uv - want).max(1) <= tol).all()
    assert (uv.min(1) >= -tol).all() and (uv.sum(1) <= 1 + tol).all()


def test_reduction_restatements():
    d = np.array([0.5, -2.0, np.inf, 0.25, -np.inf], np.float32)
    assert SO.distance_stats(d, tau=0.5) == (2.0, 2.75, 0.25 + 4.0 + 0.0625, 2, 2)
    assert SO.distance_stats(d)[3] == 0
    s, n = SO.normal_agreement(TWO_VS, TWO_FACES, [0, 1, -1, 0], TWO_VS, TWO_FACES[:, ::-1], [1, 0, 0, 0x7FFFFFFF])
    assert n == 2 and s == 2.0                      # parallel planes, one of them reversed: |cos| = 1


def test_new_entry_points_validate_without_gpu():
    """sg_sampler_* / sg_distance_stats / sg_normal_agreement refuse null pointers and bad sizes before a device is
    touched (the manner of test_capi.py::test_argument_validation_without_gpu)."""
    lib = capi.load()
    out = ctypes.c_void_p()
    buf = (ctypes.c_float * 9)()
    p = ctypes.addressof(buf)
    assert lib.sg_sampler_create(None, 3, None, 1, None, None, ctypes.byref(out)) == -1 and b"null pointer" in lib.sg_last_error()
    assert lib.sg_sampler_create(p, 3, p, 1, None, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert lib.sg_sampler_create(p, 3, p, 0, None, None, ctypes.byref(out)) == -1 and b"at least one face" in lib.sg_last_error()
    assert lib.sg_sampler_create(p, 3, p, -1, None, None, ctypes.byref(out)) == -1
    assert lib.sg_sampler_create(p, 3, p, 1 << 31, None, None, ctypes.byref(out)) == -1 and b"int32" in lib.sg_last_error()
    assert out.value is None
    assert lib.sg_sampler_destroy(None) == 0
    info = (ctypes.c_int64 * 4)()
    assert lib.sg_sampler_query(None, info) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_sampler_export(None, None, None, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_sampler_locate(None, p, 1, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_sampler_draw(None, 0, 0, 1, 0, p, p, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    for fn, args in ((lib.sg_distance_stats, lambda n: (p, n, 0.0, p, p, None)),
                     (lib.sg_normal_agreement, lambda n: (p, p, p, p, p, p, n, p, p, None))):
        assert fn(*args(-1)) == -1 and b"2^31" in lib.sg_last_error()
        assert fn(*args(1 << 31)) == -1
        assert fn(*args(0)) == 0                                  # nothing to do: no launch
    assert lib.sg_distance_stats(None, 4, 0.0, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert lib.sg_distance_stats(p, 4, 0.0, None, p, None) == -1
    assert lib.sg_distance_stats(p, 4, 0.0, p, None, None) == -1
    assert lib.sg_normal_agreement(p, p, None, p, p, p, 4, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert lib.sg_normal_agreement(p, p, p, p, p, p, 4, None, p, None) == -1
