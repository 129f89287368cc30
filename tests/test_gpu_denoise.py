"""The vertex update on the device (csrc/mesh_denoise.hip) against the numpy oracle (tests/denoise_oracle.py), bit for bit,
and the two-stage denoiser built on it (semigcn_amd/denoise.py).  The premises used here (the oracle stays within 2e-6 of
the reference, a plane is a fixed point, a + b steps, what must not move, the denoising effect) are asserted on the CPU
in tests/test_denoise_oracle.py.

  bits     sg_vupdate_run equals the oracle on the int32 views: every valence path of the kernel (below and past the four
           gathers in flight, past one wavefront of faces at a vertex), sizes one lane past a block and past four blocks,
           far coordinates with non-unit normals, a movable mask, steps = 0, 3 + 7 steps, two runs and two plans, one
           size past 1024 blocks, a NaN normal;
  the rest the reference's recorded results within 2e-6, denoise_mesh against the composition of the two public
           operations, the denoising effect on the noisy box, plan reuse, the command line."""
import json
import os

import numpy as np
import pytest
import torch

import denoise_oracle as DO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: shared inputs are read-only
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.float32 and torch.equal(bits(got.cpu()), bits(torch.from_numpy(np.array(want, np.float32))))


def random_normals(F, seed, unit=True):
    n = np.random.default_rng(seed).standard_normal((F, 3))
    if unit:
        n /= np.linalg.norm(n, axis=1, keepdims=True)
    return n.astype(np.float32)


def run_both(vs, faces, normals, steps, movable=None):
    from semigcn_amd import denoise
    got = denoise.update_vertices(dev(vs), dev(faces), dev(normals), steps, movable=None if movable is None else dev(movable))
    return got, DO.update_vertices(vs, faces, normals, steps, movable)


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def grid(n, m):
    """An open n x m grid of vertices, two triangles per cell, gently curved."""
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n - 1), np.arange(m - 1), indexing="ij"))
    a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)
    x, y = (v.reshape(-1).astype(np.float64) for v in np.meshgrid(np.arange(n), np.arange(m), indexing="ij"))
    vs = np.stack([x, y, 0.3 * np.sin(0.7 * x) * np.cos(0.4 * y)], 1).astype(np.float32)
    return vs, faces


def fan(k):
    """A closed fan of k triangles around vertex 0: the hub has valence k, the rim vertices 2."""
    t = 2 * np.pi * np.arange(k) / k
    vs = np.concatenate([[[0.0, 0.0, 0.4]], np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], 1)]).astype(np.float32)
    r = np.arange(k)
    faces = np.stack([np.zeros(k, np.int64), 1 + r, 1 + (r + 1) % k], 1).astype(np.int64)
    return vs, faces


TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0.2], [0, 1, -0.1]], np.float32), np.array([[0, 1, 2]], np.int64))
TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.2, 0.3, 1]], np.float32),
         np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64))


def with_unused():
    """The tetrahedron among vertices that no face names: the first, one in the middle and the last index."""
    vs = np.random.default_rng(5).standard_normal((8, 3)).astype(np.float32)
    faces = np.array([1, 2, 4, 5], np.int64)[TETRA[1]]
    return vs, faces


def grid257():
    """grid(3, 86) has 258 vertices; without the last one and its faces V = 257, one lane past a block."""
    vs, faces = grid(3, 86)
    return vs[:257], faces[(faces < 257).all(1)]


SMALL = {"triangle": lambda: TRIANGLE, "tetrahedron": lambda: TETRA, "unused": with_unused, "fan80": lambda: fan(80),
         "grid257": grid257, "grid1025": lambda: grid(41, 25)}


def _small(name):
    return SMALL[name]()


@pytest.mark.parametrize("name", ["triangle", "tetrahedron", "unused", "fan80", "grid257", "grid1025"])
def test_small_meshes_equal_the_oracle_bit_for_bit(name):
    from semigcn_amd import capi
    vs, faces = _small(name)
    V, F = len(vs), len(faces)
    k = np.bincount(faces.reshape(-1), minlength=V)
    expect = {"triangle": (3, 1), "tetrahedron": (4, 3), "unused": (8, 3), "fan80": (81, 80), "grid257": (257, 6),
              "grid1025": (1025, 6)}[name]
    assert (V, int(k.max())) == expect
    normals = random_normals(F, 17)
    with capi.VertexUpdatePlan(dev(faces), V) as plan:
        assert (plan.max_valence, plan.num_unused) == (int(k.max()), int((k == 0).sum()))
        for steps in (1, 4):
            got = plan.run(dev(vs), dev(normals), None, steps)
            want = DO.update_vertices(vs, faces, normals, steps)
            assert same_bits(got, want), (name, steps, np.abs(got.cpu().numpy() - want).max())
    if name == "unused":
        assert (k[[0, 3, 7]] == 0).all() and same_bits(got[[0, 3, 7]], vs[[0, 3, 7]])
    assert not np.array_equal(want, vs)


@pytest.fixture(scope="module")
def far_torus():
    """torus_mesh(60, 40) shifted by 1e4 in x, non-unit random normals, and the oracle's 10 steps (computed once)."""
    m = synth.torus_mesh(60, 40, masks=False)
    vs = m.vs.astype(np.float32)
    vs[:, 0] += np.float32(1e4)
    normals = random_normals(len(m.faces), 23, unit=False)
    want = DO.update_vertices(vs, m.faces, normals, 10)
    for a in (vs, normals, want):
        a.setflags(write=False)
    return vs, m.faces, normals, want


def test_far_coordinates_and_non_unit_normals(far_torus):
    from semigcn_amd import denoise
    vs, faces, normals, want = far_torus
    got = denoise.update_vertices(dev(vs), dev(faces), dev(normals), 10)
    assert same_bits(got, want), np.abs(got.cpu().numpy() - want).max()
    assert np.abs(want - vs).max() > 1e-2


def test_three_plus_seven_steps_equal_ten(far_torus):
    from semigcn_amd import capi
    vs, faces, normals, want = far_torus
    with capi.VertexUpdatePlan(dev(faces), len(vs)) as plan:
        mid = plan.run(dev(vs), dev(normals), None, 3)
        got = plan.run(mid, dev(normals), None, 7)
    assert same_bits(got, want)
    assert same_bits(mid, DO.update_vertices(vs, faces, normals, 3))


def test_two_runs_and_two_plans_give_identical_bits(far_torus):
    from semigcn_amd import capi
    vs, faces, normals, want = far_torus
    p, f, n = dev(vs), dev(faces), dev(normals)
    with capi.VertexUpdatePlan(f, len(vs)) as plan, capi.VertexUpdatePlan(f, len(vs)) as other:
        a, b, c = plan.run(p, n, None, 10), plan.run(p, n, None, 10), other.run(p, n, None, 10)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) and same_bits(a, want)
    assert same_bits(p, vs)                                   # the input is left alone


def test_steps_zero_copies(far_torus):
    from semigcn_amd import denoise
    vs, faces, normals, _ = far_torus
    p = dev(vs)
    got = denoise.update_vertices(p, dev(faces), dev(normals), 0)
    assert same_bits(got, vs) and got.data_ptr() != p.data_ptr()


def test_movable_mask_with_half_the_vertices_fixed(far_torus):
    vs, faces, normals, _ = far_torus
    movable = np.random.default_rng(29).random(len(vs)) < 0.5
    got, want = run_both(vs, faces, normals, 5, movable)
    assert same_bits(got, want)
    assert same_bits(got[dev(~movable)], vs[~movable]) and 0.4 < movable.mean() < 0.6
    assert (np.abs(want[movable] - vs[movable]).max(1) > 0).mean() > 0.9


def test_one_size_past_1024_blocks():
    m = synth.torus_mesh(600, 450, masks=False)
    vs = m.vs.astype(np.float32)
    assert len(vs) == 270000 > 1024 * 256
    normals = random_normals(len(m.faces), 31)
    got, want = run_both(vs, m.faces, normals, 2)
    assert same_bits(got, want), np.abs(got.cpu().numpy() - want).max()


def test_a_nan_normal_spreads_as_in_the_oracle():
    vs, faces = _small("grid1025")
    normals = random_normals(len(faces), 37)
    normals[len(faces) // 2] = np.float32("nan")
    got, want = run_both(vs, faces, normals, 2)
    g = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(g), nan)
    assert 3 < nan.any(1).sum() < 40                         # the face's corners after one step, their ring after two
    assert np.array_equal(g[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ---- the reference's recorded results -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "open"])
@pytest.mark.parametrize("loop", [1, 10])
def test_update_vertices_against_the_recorded_reference(name, loop):
    from semigcn_amd import denoise
    g6, g8 = np.load(os.path.join(GOLDEN, "g6_bnf.npz")), np.load(os.path.join(GOLDEN, "g8_vertex_update.npz"))
    want = g8[f"{name}/loop{loop}"]
    got = denoise.update_vertices(g6[f"{name}/pos"], g6[f"{name}/faces"], g6[f"{name}/new_fn"], loop).cpu().numpy()
    rel = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print(f"{name} loop {loop}: max |device - reference| / max |coordinate| = {rel:.3g} (bound 2e-6)")
    assert rel <= 2e-6


# ---- the denoiser ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    return DO.noisy_box(12, 0.12, 7)


def test_denoise_mesh_is_the_composition_of_the_two_public_operations(box):
    from semigcn_amd import capi, denoise, functional, train
    _, noisy, faces = box
    p, f = dev(noisy), dev(faces)
    movable = dev(np.random.default_rng(41).random(len(noisy)) < 0.9)
    out = denoise.denoise_mesh(p, f, iterations=2, normal_rounds=4, sigma_s=0.35, vertex_steps=6, movable=movable)
    f2f = capi.mesh_edges(f, len(noisy), with_f2f=True)[1]
    q, residual = p, []
    for _ in range(2):
        fn = train.face_normals(q, f)                                               # the face normals going in
        n = functional.bilateral_normal_filter(q, f, f2f, loop=4, sigma_s=0.35)
        residual.append(float((n - fn).abs().sum().double() / len(faces)))
        q = denoise.update_vertices(q, f, n, 6, movable=movable)
    assert torch.equal(bits(out.vs), bits(q)) and torch.equal(bits(out.normals), bits(n))
    r = out.report
    assert (r["n_vertices"], r["n_faces"], r["n_unused"], r["max_valence"]) == (866, 1728, 0, int(np.bincount(faces.reshape(-1)).max()))
    # two float32 evaluations of a sum of 3 F = 5184 terms: n eps = 3e-4 relative at the worst
    assert len(r["normal_residual"]) == 2 and np.allclose(r["normal_residual"], residual, rtol=1e-3) and out.stage_ms is None
    assert r["normal_residual"][1] < r["normal_residual"][0]
    with_f2f = denoise.denoise_mesh(p, f, iterations=2, normal_rounds=4, sigma_s=0.35, vertex_steps=6, movable=movable, f2f=f2f,
                                    timings=True)
    assert torch.equal(bits(with_f2f.vs), bits(q)) and set(with_f2f.stage_ms) == {"topology_ms", "plan_ms", "filter_ms", "update_ms"}


def test_one_iteration_halves_the_normal_angle_on_the_noisy_box(box):
    from semigcn_amd import denoise
    clean, noisy, faces = box
    before = DO.mean_normal_angle(noisy, faces, clean)
    out = denoise.denoise_mesh(noisy, faces, iterations=1)
    after = DO.mean_normal_angle(out.vs.cpu().numpy(), faces, clean)
    print(f"mean normal angle on the device: {before:.2f} deg -> {after:.2f} deg after one iteration (float32 on the CPU: "
          "13.61 deg -> 2.93 deg in tests/test_denoise_oracle.py; 14.48 deg -> 3.29 deg with the noise of the first study)")
    assert after <= 0.5 * before
    assert out.normals.shape == (len(faces), 3) and out.report["iterations"] == 1


def test_a_plan_is_reused_across_calls_and_a_closed_plan_raises(box):
    from semigcn_amd import capi, denoise
    _, noisy, faces = box
    p, f = dev(noisy), dev(faces)
    plan = capi.VertexUpdatePlan(f, len(noisy))
    h = plan._h.value
    a = denoise.denoise_mesh(p, f, iterations=3, plan=plan)
    b = denoise.denoise_mesh(p, f, iterations=3)
    assert plan._h.value == h and torch.equal(bits(a.vs), bits(b.vs))
    n = dev(random_normals(len(faces), 43))
    assert torch.equal(bits(denoise.update_vertices(p, f, n, 2, plan=plan)), bits(denoise.update_vertices(p, f, n, 2)))
    with pytest.raises(capi.SemigcnLibraryError, match="plan of 866 vertices"):
        denoise.update_vertices(p[:800], f[:10], n[:10], 2, plan=plan)
    with pytest.raises(capi.SemigcnLibraryError, match="normals must be float32"):
        plan.run(p, n[:-1])
    torch.cuda.synchronize()
    plan.close()
    with pytest.raises(capi.SemigcnLibraryError, match="VertexUpdatePlan is closed"):
        plan.run(p, n)
    with pytest.raises(capi.SemigcnLibraryError, match="closed"):
        denoise.update_vertices(p, f, n, 2, plan=plan)


def test_invalid_faces_are_refused():
    from semigcn_amd import capi
    with pytest.raises(capi.SemigcnLibraryError, match=r"outside \[0, 4\)"):
        capi.VertexUpdatePlan(dev(np.array([[0, 1, 4]], np.int64)), 4)
    with pytest.raises(capi.SemigcnLibraryError, match="repeated vertex"):
        capi.VertexUpdatePlan(dev(np.array([[0, 1, 2], [2, 3, 2]], np.int64)), 4)
    with capi.VertexUpdatePlan(dev(np.zeros((0, 3), np.int64)), 5) as plan:
        assert (plan.max_valence, plan.num_unused) == (0, 5)
        p = dev(np.arange(15, dtype=np.float32).reshape(5, 3))
        assert torch.equal(plan.run(p, dev(np.zeros((0, 3), np.float32)), None, 3), p)


def test_command_line(capsys):
    from semigcn_amd import denoise
    assert denoise.main(["--box", "12", "--noise", "0.12", "--iterations", "2", "--repeat", "2"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["n_vertices"], rec["n_faces"], rec["n_unused"], rec["iterations"]) == (866, 1728, 0, 2)
    assert {"topology_ms", "plan_ms", "filter_ms", "update_ms"} <= set(rec) and len(rec["normal_residual"]) == 2
    assert rec["normal_angle_after_deg"] <= 0.5 * rec["normal_angle_before_deg"]
