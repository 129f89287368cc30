"""The numpy oracle of the vertex update (tests/denoise_oracle.py) against the reference's recorded results, and the
premises the device tests of tests/test_gpu_denoise.py build on, on the CPU.

The bound: 2e-6 relative to the largest coordinate, the bound tests/test_gpu_bnf.py holds the reference's filter to.  The
reference evaluates the same sums in another order (torch.sum over the three components and over the faces of a vertex),
which is worth a few float32 roundings of numbers below the coordinates: 3e-8 observed."""
import os

import numpy as np
import pytest
import torch

import denoise_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND = 2e-6


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["sphere", "open"])
@pytest.mark.parametrize("loop", [1, 10])
def test_oracle_against_the_recorded_reference(name, loop):
    g6, g8 = _g("g6_bnf.npz"), _g("g8_vertex_update.npz")
    want = g8[f"{name}/loop{loop}"]
    got = DO.update_vertices(g6[f"{name}/pos"], g6[f"{name}/faces"], g6[f"{name}/new_fn"], loop)
    rel = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print(f"{name} loop {loop}: max |oracle - reference| / max |coordinate| = {rel:.3g} (bound {BOUND})")
    assert want.dtype == np.float32 and want.shape == got.shape
    assert rel <= BOUND
    assert np.abs(want - g6[f"{name}/pos"]).max() > 100 * BOUND * np.abs(want).max()      # the update moved something


def test_golden_holds_results_only():
    g8 = _g("g8_vertex_update.npz")
    assert sorted(g8.files) == sorted(f"{n}/loop{k}" for n in ("sphere", "open") for k in (1, 10))
    assert os.path.getsize(os.path.join(GOLDEN, "g8_vertex_update.npz")) < 32 * 1024


def test_oracle_against_the_live_reference():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference tree is not present")
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_golden_denoise", os.path.join(os.path.dirname(GOLDEN), os.pardir, "tools", "make_golden_denoise.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g6, g8 = _g("g6_bnf.npz"), _g("g8_vertex_update.npz")
    live = tool.reference_results(g6)
    for key, want in live.items():
        name, loop = key.split("/")[0], int(key.split("loop")[1])
        got = DO.update_vertices(g6[f"{name}/pos"], g6[f"{name}/faces"], g6[f"{name}/new_fn"], loop)
        rel = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        print(f"{key}: max |oracle - live reference| / max |coordinate| = {rel:.3g}")
        assert rel <= BOUND
        assert np.array_equal(_bits(want), _bits(g8[key])), key          # the fixture is what the reference gives today


# ---- premises ------------------------------------------------------------------------------------------------------------
def _grid(n):
    """An open n x n grid of vertices in the plane z = 0.5 (float32), two triangles per cell."""
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij"))
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)
    x, y = (v.reshape(-1) for v in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    vs = np.stack([x * 0.37, y * 0.61, np.full(n * n, 0.5)], 1).astype(np.float32)
    return vs, faces


def test_a_plane_with_its_normals_is_a_bit_exact_fixed_point():
    vs, faces = _grid(9)
    normals = np.tile(np.array([0, 0, 1], np.float32), (len(faces), 1))
    out = DO.update_vertices(vs, faces, normals, 7)
    assert np.array_equal(_bits(out), _bits(vs))


def _sphere_case():
    g6 = _g("g6_bnf.npz")
    return g6["open/pos"], g6["open/faces"], g6["open/new_fn"]


def test_a_plus_b_steps_equal_a_then_b():
    pos, faces, fn = _sphere_case()
    whole = DO.update_vertices(pos, faces, fn, 10)
    parts = DO.update_vertices(DO.update_vertices(pos, faces, fn, 3), faces, fn, 7)
    assert np.array_equal(_bits(whole), _bits(parts))
    assert not np.array_equal(_bits(whole), _bits(DO.update_vertices(pos, faces, fn, 9)))


def test_immovable_and_unused_vertices_keep_their_bits():
    pos, faces, fn = _sphere_case()
    pos = np.concatenate([pos, np.array([[3.5, -1.25, 0.1], [9.0, 9.0, 9.0]], np.float32)])      # two vertices without a face
    V = len(pos)
    movable = np.random.default_rng(3).random(V) < 0.5
    out = DO.update_vertices(pos, faces, fn, 4, movable)
    free = DO.update_vertices(pos, faces, fn, 4)
    assert np.array_equal(_bits(out[~movable]), _bits(pos[~movable]))
    assert np.array_equal(_bits(out[-2:]), _bits(pos[-2:])) and np.array_equal(_bits(free[-2:]), _bits(pos[-2:]))
    moved = movable[:-2] & (np.abs(out[:-2] - pos[:-2]).max(1) > 0)
    assert moved.sum() > 0.4 * movable.sum()
    # a fixed vertex still feeds the centroids: its movable neighbours end elsewhere than in the run where all move
    assert not np.array_equal(_bits(out[movable]), _bits(free[movable]))


def test_one_iteration_halves_the_normal_angle_on_the_noisy_box_and_a_laplacian_step_does_not():
    from oracle import meshprep as OM
    from semigcn_amd import train
    clean, noisy, faces = DO.noisy_box(12, 0.12, 7)
    assert len(clean) == 866
    f2f = OM.face_ring(faces, len(clean))
    before = DO.mean_normal_angle(noisy, faces, clean)
    p = torch.from_numpy(noisy)
    ft, rt = torch.from_numpy(faces), torch.from_numpy(np.asarray(f2f, np.int64))
    filtered = train.bilateral_normal_loss(p, train.face_normals(p, ft), ft, rt, loop=5, sigma_s=0.3)[1]
    after = DO.mean_normal_angle(DO.update_vertices(noisy, faces, filtered.numpy(), 10), faces, clean)
    lap = DO.mean_normal_angle(DO.laplacian_step(noisy, faces), faces, clean)
    print(f"mean normal angle: noisy {before:.2f} deg, one iteration {after:.2f} deg, one Laplacian step {lap:.2f} deg")
    assert after <= 0.5 * before
    assert lap > 0.5 * before
