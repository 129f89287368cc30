"""Registration on the device (semigcn_amd/align.py, csrc/mesh_align.hip): the transform against the numpy restatement bit
for bit, the normal equations against its exact sums within the bound of any summation order, ``align`` end to end against
the figure of the float64 run (tests/align_fixtures.py, ``E_O``), and the ``--align`` option of the scorer's command line.

The figures in the docstrings below were measured on an MI355X; every test prints its own."""
import json
import math

import numpy as np
import pytest
import torch

import align_fixtures as AF
import align_oracle as AO
from semigcn_amd import align, capi, evaluate, mesh_common

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
BOUND = 4 * AF.E_O


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype)


def _target(name):
    if name == "tetrahedron":
        return AF.tetrahedron()
    if name == "tetrahedron_zero":          # a zero-area face (a repeated vertex) on a segment of its own, beside the body
        vs, faces = AF.tetrahedron()
        vs = np.concatenate([vs, np.array([[2.0, 2.0, 0.5], [2.5, 2.0, 1.0]], np.float32)])
        return vs, np.concatenate([np.array([[4, 5, 5]], np.int64), faces])
    return AF.lumpy_torus()


def _points(vs, n, seed, sigma=0.25):
    rng = np.random.default_rng(seed)
    return (vs[rng.integers(0, len(vs), n)] + rng.normal(0.0, sigma, (n, 3))).astype(np.float32)


# ---- transform ----

@pytest.mark.parametrize("n", [1, 65, 1025])
def test_transform_equals_the_oracle_bit_for_bit(n):
    rng = np.random.default_rng(n)
    pts = rng.normal(0.0, 2.0, (n, 3)).astype(np.float32)
    pts[::3] += np.float32(1e4)                                      # coordinates near 1e4
    if n > 1:
        pts[n // 2] = [np.nan, 1.0, np.inf]
    for S in (AF.similarity(None), AF.similarity(n, False), np.eye(4)):
        ref = AO.transform(S, pts)
        out = capi.align_transform(_t(pts), S)
        assert out.dtype == torch.float32 and out.shape == (n, 3)
        assert np.array_equal(out.cpu().numpy(), ref, equal_nan=True)
        assert n == 1 or np.isnan(ref[n // 2]).all()                # the NaN row stays one, the others are untouched
        buf = _t(pts)                                               # in place
        assert capi.align_transform(buf, S, out=buf) is buf and np.array_equal(buf.cpu().numpy(), ref, equal_nan=True)
        assert np.array_equal(align.apply(S, pts).cpu().numpy(), ref, equal_nan=True)
    nan = capi.align_transform(_t([[np.nan, 0.0, 0.0]]), AF.similarity(None)).cpu().numpy()
    assert np.isnan(nan).all()
    assert capi.align_transform(_t(np.zeros((0, 3))), np.eye(4)).shape == (0, 3)


# ---- accumulate ----

def _accumulate(name, pts, S, with_scale, max_dist=math.inf, edit=None):
    """(device out, oracle out, oracle sums of |term|, face) with closest / face / dist from the device's own query."""
    vs, faces = _target(name)
    dvs, dfaces = _t(vs), _t(faces, torch.int64)
    with capi.SurfaceHandle(dvs, dfaces) as h:
        dist, face, closest = h.query(capi.align_transform(_t(pts), S), signed=False)
    if edit is not None:
        edit(face)
    dev = capi.align_accumulate(dvs, dfaces, _t(pts), S, closest, face, dist, max_dist, with_scale)
    again = capi.align_accumulate(dvs, dfaces, _t(pts), S, closest, face, dist, max_dist, with_scale)
    assert torch.equal(dev.view(torch.int64), again.view(torch.int64))          # two runs: identical bytes
    ref, sabs = AO.accumulate(vs, faces, pts, S, closest.cpu().numpy(), face.cpu().numpy(), dist.cpu().numpy(), max_dist,
                              with_scale, with_abs=True)
    return dev.cpu().numpy(), ref, sabs, face.cpu().numpy()


def _check(dev, ref, sabs, with_scale):
    assert dev.shape == (40,) and np.array_equal(dev[37:], ref[37:]), (dev[37:], ref[37:])
    n = int(ref[37])
    err, bound = np.abs(dev[:37] - ref[:37]), (n + 16) * EPS * sabs
    assert (err <= bound).all(), (n, np.nonzero(err > bound)[0], err, bound)
    if not with_scale:
        assert not dev[[6, 12, 17, 21, 24, 26, 27, 34]].any()                    # row and column 6: exactly zero
    return float((err / np.where(bound > 0, bound, 1.0)).max())


@pytest.mark.parametrize("with_scale", [0, 1])
@pytest.mark.parametrize("name", ["tetrahedron", "torus"])
def test_accumulate_sizes(name, with_scale):
    """The sums stay within the derived bound at every size.  Measured: at most 1.4 % of the bound is used."""
    vs = _target(name)[0]
    worst = 0.0
    for n in (1, 2, 63, 64, 65, 257, 1025, 3077):
        pts = _points(vs, n, 100 + n)
        dev, ref, sabs, _ = _accumulate(name, pts, AF.similarity(n, bool(with_scale)), with_scale)
        assert ref[37] == n and ref[38] == 0 and ref[39] == 0
        worst = max(worst, _check(dev, ref, sabs, with_scale))
    print(f"{name} with_scale={with_scale}: largest |S_dev - S_fsum| / bound = {worst:.3f}")


def test_accumulate_past_the_block_cap():
    """N = 2^18 + 3: 1024 blocks of 512 rows, two rows per lane.  Measured: below 0.01 % of the bound."""
    n = (1 << 18) + 3
    pts = _points(_target("torus")[0], n, 9)
    dev, ref, sabs, _ = _accumulate("torus", pts, AF.similarity(9), 1)
    assert ref[37] == n
    print(f"N = {n}: largest |S_dev - S_fsum| / bound = {_check(dev, ref, sabs, 1):.4f}")


@pytest.mark.parametrize("with_scale", [0, 1])
def test_accumulate_rejects_and_skips(with_scale):
    vs = _target("torus")[0]
    n = 1025
    pts = _points(vs, n, 3)
    S = AF.similarity(5, bool(with_scale))
    # a max_dist in the middle of the distances, and one that rejects every row
    dev, ref, sabs, _ = _accumulate("torus", pts, S, with_scale, max_dist=0.2)
    assert 100 < ref[37] < n - 100 and ref[37] + ref[38] == n and ref[39] == 0
    _check(dev, ref, sabs, with_scale)
    dev, ref, sabs, _ = _accumulate("torus", pts, S, with_scale, max_dist=0.0)
    assert not dev[:38].any() and dev[38] == n and dev[39] == 0 and np.array_equal(dev, ref)
    # NaN points (the first, one inside, the last) and rows without a face
    pts[[0, 517, n - 1]] = np.nan
    pts[300, 1] = np.inf

    def edit(face):
        face[[5, 640]] = capi.NO_FACE
        face[77] = -1
    dev, ref, sabs, face = _accumulate("torus", pts, S, with_scale, edit=edit)
    assert (face[[0, 517, n - 1, 300]] == capi.NO_FACE).all()
    assert ref[39] == 7 and ref[38] == 0 and ref[37] == n - 7 and np.isfinite(dev).all()
    _check(dev, ref, sabs, with_scale)


def test_accumulate_skips_a_zero_area_face():
    vs, faces = _target("tetrahedron_zero")
    rng = np.random.default_rng(2)
    near = (vs[4] + rng.uniform(0, 1, (40, 1)) * (vs[5] - vs[4]) + rng.normal(0, 0.05, (40, 3))).astype(np.float32)
    pts = np.concatenate([_points(vs[:4], 200, 4), near])
    for ws in (0, 1):
        dev, ref, sabs, face = _accumulate("tetrahedron_zero", pts, AF.similarity(6, bool(ws)), ws)
        assert (face == 0).sum() >= 30 and ref[39] == (face == 0).sum() and ref[37] == len(pts) - ref[39]
        _check(dev, ref, sabs, ws)


# ---- align, end to end ----

def _error(a, src, vs, bound=BOUND, rows=None):
    moved = align.apply(a.matrix, src).cpu().numpy().astype(np.float64)
    rows = slice(None) if rows is None else rows
    err = float(np.linalg.norm(moved[rows] - np.asarray(vs, np.float64), axis=1).max())
    print(f"  {a.iterations} iterations, reason {a.reason}, rms {a.rms:.3e}, point error {err:.3e} (bound {bound:.3e})")
    assert a.converged and a.reason == "converged" and a.iterations <= 10
    assert err <= bound, (err, bound)
    return err


@pytest.mark.parametrize("with_scale", [False, True])
def test_align_recovers_the_similarity(with_scale):
    """Vertices of the lumpy torus under the fixture's similarity onto the torus: within 4 E_O = 6.8e-7 of its vertices.
    Measured: 4 iterations, 1.38e-7 rigid and 1.33e-7 with scale (the float64 run: 1.37e-7 and 1.69e-7)."""
    vs, faces = AF.lumpy_torus()
    S = AF.similarity(None, with_scale)
    src = AF.moved(S, vs)
    a = align.align((src, faces), (vs, faces), points="vertices", with_scale=with_scale, timings=True)
    _error(a, src, vs)
    assert np.abs(a.matrix @ S - np.eye(4)).max() <= 1e-6
    assert abs(a.scale - 1.0 / (1.07 if with_scale else 1.0)) <= 1e-6 and np.array_equal(a.translation, a.matrix[:3, 3])
    assert np.abs(a.rotation @ a.rotation.T - np.eye(3)).max() <= 1e-12 and np.array_equal(a.matrix[3], [0, 0, 0, 1])
    assert len(a.history) == a.iterations and all(h["n_used"] == 200 and h["n_far"] == 0 and h["n_skipped"] == 0 for h in a.history)
    assert a.history[-1]["step"] <= 1e-6 and a.rms == a.history[-1]["rms"] and a.rms < 1e-5
    assert set(a.stage_ms) == {"sample_ms", "transform_ms", "query_ms", "accumulate_ms"}
    # the same on a Surface that the caller keeps, without timings
    with evaluate.Surface(vs, faces) as s:
        b = align.align((src, faces), s, points="vertices", with_scale=with_scale)
        assert b.stage_ms is None and np.array_equal(a.matrix, b.matrix) and a.history == b.history       # two runs: identical
        assert s.query(_t(vs))[0].shape == (200,)                   # the caller's surface is still open


@pytest.mark.parametrize("with_scale", [False, True])
def test_align_from_the_centroids(with_scale):
    """A translation of three box diagonals first: ``init="centroid"`` takes it out.  The source's coordinates are then
    near 17 instead of 3, and a float32 there has a spacing 8 times as large: the rounding of the source, which is what
    E_O consists of, grows by that factor, and so does the bound (computed from the two spacings, not measured): 5.44e-6.
    Measured: 4 iterations, 1.15e-6 rigid and 1.02e-6 with scale (the float64 run: 1.14e-6 and 1.05e-6)."""
    vs, faces = AF.lumpy_torus()
    S = AF.similarity(None, with_scale)
    S[:3, 3] += 3.0 * AO.box_diagonal(vs) / math.sqrt(3.0)
    src = AF.moved(S, vs)
    factor = float(np.spacing(np.abs(src).max()) / np.spacing(np.abs(AF.moved(AF.similarity(None, with_scale), vs)).max()))
    assert factor == 8.0
    a = align.align((src, faces), (vs, faces), points="vertices", with_scale=with_scale, init="centroid")
    _error(a, src, vs, bound=BOUND * factor)


def test_align_samples_of_a_cut_source():
    """The source has lost 30 % of its faces in one patch and is sampled (n = 4096); the target is whole.  Measured: 5
    iterations, 1.33e-7 to 2.39e-7 over the two sample streams, rigid and with scale."""
    vs, faces = AF.lumpy_torus()
    cut = AF.cut_faces(vs, faces)
    for ws in (False, True):
        S = AF.similarity(None, ws)
        src = AF.moved(S, vs)
        a = align.align((src, cut), (vs, faces), points="samples", n=4096, with_scale=ws)
        _error(a, src, vs)
        assert all(h["n_used"] == 4096 for h in a.history)
        b = align.align((src, cut), (vs, faces), points="samples", n=4096, with_scale=ws, seed=1)
        assert not np.array_equal(a.matrix, b.matrix)              # another sample stream, another last bit
        _error(b, src, vs)


def test_align_leaves_out_a_far_component():
    """23 points of clutter 48 away, ``max_dist=1.5``: counted in ``n_far`` and without effect (measured: 1.38e-7, the figure
    of the run without them); without ``max_dist`` they pull the pose away."""
    vs, faces = AF.lumpy_torus()
    S = AF.similarity(None, False)
    far = (np.random.default_rng(8).normal(0, 0.3, (23, 3)) + [30.0, -25.0, 28.0]).astype(np.float32)
    src = np.concatenate([AF.moved(S, vs), far])
    a = align.align((src, faces), (vs, faces), points="vertices", max_dist=1.5)
    _error(a, src, vs, rows=slice(0, 200))
    assert all(h["n_far"] == 23 and h["n_used"] == 200 and h["n_skipped"] == 0 for h in a.history)
    b = align.align((src, faces), (vs, faces), points="vertices", max_iter=10)        # without max_dist the clutter pulls
    assert np.abs(b.matrix @ S - np.eye(4)).max() > 1e-3


def test_align_reports_a_degenerate_target_and_the_iteration_cap():
    gv, gf = AF.flat_grid()
    src = AF.moved(AF.similarity(None, False), gv)
    for ws in (False, True):
        a = align.align((src, gf), (gv, gf), points="vertices", with_scale=ws)
        assert a.reason == "degenerate" and not a.converged and a.iterations == 1 and np.array_equal(a.matrix, np.eye(4))
        assert math.isnan(a.history[0]["step"]) and a.history[0]["n_used"] == 36 and np.isfinite(a.rms)
    tv, tf = AF.tetrahedron()                                      # fewer rows than unknowns
    a = align.align((tv, tf), (tv, tf), points="vertices", with_scale=False)
    assert a.reason == "degenerate" and a.history[0]["n_used"] == 4
    vs, faces = AF.lumpy_torus()
    S = AF.similarity(None)
    src = AF.moved(S, vs)
    one = align.align((src, faces), (vs, faces), points="vertices", with_scale=True, max_iter=1)
    assert not one.converged and one.reason == "max_iter" and one.iterations == 1 and len(one.history) == 1
    assert not np.array_equal(one.matrix, np.eye(4)) and np.isfinite(one.matrix).all()
    init = AF.similarity(3)
    for kw in ({"init": init}, {"init": torch.from_numpy(init)}, {}):
        zero = align.align((src, faces), (vs, faces), points="vertices", with_scale=True, max_iter=0, **kw)
        assert np.array_equal(zero.matrix, kw["init"] if kw else np.eye(4)) and zero.iterations == 0 and not zero.converged
        assert zero.reason == "max_iter" and zero.history == [] and math.isnan(zero.rms)
    # a start at the answer converges at once
    done = align.align((src, faces), (vs, faces), points="vertices", with_scale=True, init=align.inverse(S))
    assert done.converged and done.iterations <= 2


def test_align_twice_gives_identical_bytes():
    vs, faces = AF.lumpy_torus()
    src = AF.moved(AF.similarity(4), vs)
    for kw in ({"points": "vertices"}, {"points": "samples", "n": 3000, "init": "centroid"}):
        a = align.align((src, faces), (vs, faces), with_scale=True, **kw)
        b = align.align((_t(src), _t(faces, torch.int64)), (vs, faces), with_scale=True, **kw)
        assert a.matrix.tobytes() == b.matrix.tobytes() and a.history == b.history and a.iterations == b.iterations
        assert a.converged and a.iterations <= 10


# ---- the scorer's command line ----

def test_evaluate_command_line_aligns_first(tmp_path, capsys):
    """gt in one frame, out (a one-ring of faces missing) and org (a tenth of the faces missing) in another."""
    vs, faces = AF.lumpy_torus(40, 20)
    S = AF.similarity(None)
    out_f, org_f = AF.without_ring(faces, 417), AF.cut_faces(vs, faces, 0.1, at=100)
    files = {}
    for frame, v in (("same", vs), ("moved", AF.moved(S, vs))):
        for name, f in (("out", out_f), ("org", org_f)):
            files[frame, name] = str(tmp_path / f"{name}_{frame}.obj")
            mesh_common.write_obj(files[frame, name], v, f)
    gt = str(tmp_path / "gt.obj")
    mesh_common.write_obj(gt, vs, faces)

    def run(frame, *extra):
        assert evaluate.main(["--gt", gt, "--org", files[frame, "org"], "--out", files[frame, "out"], *extra]) == 0
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    same, moved, aligned = run("same"), run("moved"), run("moved", "--align", "similarity")
    with capsys.disabled():
        print(f"\n  hd_all * diag: same frame {same['hd_all'] * same['diag']:.6e}, moved {moved['hd_all'] * same['diag']:.3e}, "
              f"aligned {aligned['hd_all'] * same['diag']:.6e} ({aligned['align_iterations']} iterations)")
    assert list(same) == list(moved) == ["hd_all", "hd_hole", "n_hole", "diag"]
    assert list(aligned) == ["hd_all", "hd_hole", "n_hole", "diag", "align_scale", "align_iterations", "align_converged"]
    assert same["hd_all"] > 0 and moved["hd_all"] >= 100 * same["hd_all"]
    assert abs(aligned["hd_all"] - same["hd_all"]) * same["diag"] <= BOUND
    assert aligned["n_hole"] == same["n_hole"] > 0 and abs(aligned["hd_hole"] - same["hd_hole"]) * same["diag"] <= BOUND
    assert aligned["align_converged"] and aligned["align_iterations"] <= 10 and abs(aligned["align_scale"] - 1 / 1.07) <= 1e-6
    rigid = run("same", "--align", "rigid")
    assert rigid["align_scale"] == pytest.approx(1.0, abs=1e-12) and rigid["align_converged"]
    assert abs(rigid["hd_all"] - same["hd_all"]) * same["diag"] <= BOUND


def test_align_command_line(capsys):
    assert align.main(["--torus", "24", "16", "--perturb", "3", "--scale", "--vertices"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {"matrix", "scale", "iterations", "converged", "reason", "rms", "matrix_error", "transform_ms", "query_ms",
            "accumulate_ms"} <= set(line)
    assert np.asarray(line["matrix"]).shape == (4, 4) and line["iterations"] >= 1 and line["reason"] in ("converged", "max_iter")
