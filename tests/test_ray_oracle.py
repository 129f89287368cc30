"""The premises of the ray rule (semigcn_amd/render.py, "The rule"), checked on the numpy oracle without a device: it equals
exact arithmetic on integer data, it loses no ray at a vertex, an edge or a centroid, a line crosses a closed surface an
even number of times, and a tree walk that prunes by the slab interval alone equals brute force.  Beside them the two image
writers and the integer average of the supersampling."""
import numpy as np
import pytest

import ray_fixtures as RF
from ray_fixtures import read_png
import ray_oracle as R


def test_numpy_equals_exact_arithmetic_on_the_integer_box():
    vs, faces, o, d, exact = RF.int_box()
    assert faces.shape == (768, 3) and vs.min() == 0 and vs.max() == 8 and np.array_equal(vs, np.rint(vs))
    got = R.ray_cast(vs, faces, o, d)
    RF.assert_rows_equal(got, exact, "integer box", zero_sign=False)
    t, face, _ = got
    assert (face != R.NO_FACE).sum() >= len(o) - 2 and (t == 1.5).sum() >= 20 and (t == 3.0).sum() >= 20
    assert face[[np.flatnonzero((o == (20, 20, 20)).all(1))[0]]] == R.NO_FACE        # the ray that points away


@pytest.mark.parametrize("inside", [True, False])
def test_no_ray_is_lost_at_a_vertex_an_edge_or_a_centroid(inside):
    """0 misses, and the face reported is one of those that share the feature.  It is the LOWEST id among them only where
    they tie exactly at the first hit (test_gpu_ray.py's copies of one face); the float32 ray through a vertex passes beside
    it, and the figure printed below -- observed, not asserted: 44 % of the vertices from inside, 32 % from outside -- is how
    often the face it enters is also the lowest incident one."""
    vs, faces = RF.mesh("sphere")
    o, d, sharing = RF.feature_rays("sphere", inside)
    assert len(o) == 258 + 768 + 512
    _, face, _ = R.ray_cast(vs, faces, o, d)
    assert (face == R.NO_FACE).sum() == 0                                       # 0 misses
    for i, ids in enumerate(sharing):
        assert face[i] in ids, (i, face[i], ids)
    lowest = np.mean([face[i] == sharing[i].min() for i in range(258)])
    print(f"rays through the 258 vertices ({'inside' if inside else 'outside'}): {lowest:.0%} report the lowest incident face")


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_a_line_crosses_a_closed_surface_an_even_number_of_times(name):
    vs, faces = RF.mesh(name)
    o, d = RF.random_lines(name, 600, seed=1)
    hit = R.hits(vs, faces, o, d, -np.inf, np.inf)[0]
    count = hit.sum(1)
    assert (count % 2 == 0).all(), np.flatnonzero(count % 2)
    assert (count > 0).sum() > 100                                              # the lines do meet the surface


def _random_tree(n_groups, rng):
    nodes = list(range(n_groups))
    while len(nodes) > 1:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b, a = nodes.pop(j), nodes.pop(i)
        nodes.append((a, b))
    return nodes[0]


@pytest.mark.parametrize("name", ["sphere", "torus", "box", "copies"])
def test_a_walk_that_prunes_by_the_slab_interval_equals_brute_force(name):
    rng = np.random.default_rng(11)
    if name == "box":
        vs, faces, o, d, _ = RF.int_box()
        o, d = o[::5], d[::5]
    elif name == "copies":
        vs, faces = RF.one_face_copies(37)
        o = np.array([[0.5, 0.5, 3], [1, 1, 3], [0, 0, -2], [2, 0, 1], [0.5, 0.5, 0], [5, 5, 5]], np.float32)
        d = np.array([[0, 0, -1], [0, 0, -2], [0, 0, 1], [0, 0, -1], [0.25, 0.25, 0], [1, 0, 0]], np.float32)
    else:
        vs, faces = RF.mesh(name)
        o, d = RF.random_lines(name, 24, seed=3)
        fo, fd, _ = RF.feature_rays("sphere", True) if name == "sphere" else (o[:0], d[:0], None)
        o, d = np.concatenate([o, fo[::96]]), np.concatenate([d, fd[::96]])
    order = rng.permutation(len(faces))                                         # shuffled leaves of 4 faces
    groups = [order[i:i + 4] for i in range(0, len(order), 4)]
    tree = _random_tree(len(groups), rng) if len(groups) > 1 else 0
    for t_min, t_max in ((0.0, np.inf), (-np.inf, 3.0)) if name != "copies" else ((0.0, np.inf), (1.5, 3.0)):
        want = R.ray_cast(vs, faces, o, d, t_min, t_max)
        got = R.tree_cast(vs, faces, groups, tree, o, d, t_min, t_max)
        RF.assert_rows_equal(got, want, f"{name} [{t_min}, {t_max}]")
    if name == "copies":
        t, face, _ = R.ray_cast(vs, faces, o, d)
        assert list(face) == [0, 0, 0, 0, R.NO_FACE, R.NO_FACE]          # the lowest of the 37 equal faces


def test_rows_without_a_ray():
    vs, faces = RF.mesh("sphere")
    o = np.zeros((5, 3), np.float32)
    d = np.tile(vs[7], (5, 1))
    o[1, 0], d[2, 1], d[3] = np.nan, np.inf, 0.0
    t, face, bary = R.ray_cast(vs, faces, o, d)
    assert list(face[[1, 2, 3]]) == [R.NO_FACE] * 3 and np.isinf(t[[1, 2, 3]]).all() and np.isnan(bary[[1, 2, 3]]).all()
    assert face[0] == face[4] != R.NO_FACE and t[0] == t[4] and np.isfinite(bary[[0, 4]]).all()


# ---- the image writers ---------------------------------------------------------------------------------------------------

def test_png_and_apng_round_trip(tmp_path):
    import torch
    from semigcn_amd import render
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    render.write_png(str(tmp_path / "a.png"), img)
    got, delays = read_png(str(tmp_path / "a.png"))
    assert np.array_equal(got, img[None]) and delays == []
    render.write_png(str(tmp_path / "b.png"), torch.from_numpy(img[:1, :1]))
    assert np.array_equal(read_png(str(tmp_path / "b.png"))[0][0], img[:1, :1])
    frames = rng.integers(0, 256, (4, 3, 6, 3), dtype=np.uint8)
    render.write_apng(str(tmp_path / "c.png"), frames, delay_ms=70)
    got, delays = read_png(str(tmp_path / "c.png"))
    assert np.array_equal(got, frames) and delays == [70] * 4
    for bad in (img.astype(np.float32), img[..., :2], img[None], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            render.write_png(str(tmp_path / "x.png"), bad)
    with pytest.raises(ValueError, match="delay_ms"):
        render.write_apng(str(tmp_path / "x.png"), frames, delay_ms=-1)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_the_integer_average_of_the_supersampling(s):
    import torch
    from semigcn_amd import render
    rng = np.random.default_rng(s)
    big = rng.integers(0, 256, (3 * s, 5 * s, 3), dtype=np.uint8)
    big[:s, :s] = 255                                        # a block of the top level must not overflow
    big[:s, s:2 * s] = [[[0, 1, 255]]]
    want = R.ssaa_average(big, s)
    exact = np.floor(big.astype(np.float64).reshape(3, s, 5, s, 3).sum((1, 3)) / (s * s) + 0.5)
    ties = (big.astype(np.int64).reshape(3, s, 5, s, 3).sum((1, 3)) * 2 + s * s) % (2 * s * s) == 0
    assert np.array_equal(want[~ties], exact[~ties].astype(np.uint8)) and (want[0, 0] == 255).all()
    got = render._downsample(torch.from_numpy(big), s)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
