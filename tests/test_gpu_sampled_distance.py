"""The sampler and the two-sided sampled distance (semigcn_amd.evaluate.sample_surface / surface_distance,
csrc/mesh_sample.hip): bit equality with the numpy restatement of the sampling rule (tests/sample_oracle.py), the distances
against the float64 closest-point oracle (tests/mesh_distance_oracle.py), and what the reference's one-sided vertex mean
cannot see."""
import json
import math

import numpy as np
import pytest
import torch

import mesh_distance_oracle as MO
import sample_oracle as SO
from semigcn_amd import capi, evaluate, mesh_common, synth
from semigcn_amd.capi import SemigcnLibraryError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_HI = (0xC0FFEE11 << 32) | 0x9E3779B9          # a seed with high bits
NS = (1, 63, 64, 65, 255, 256, 257, 1025)
EPS = 2.0 ** -52


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype)


def _zero_run_mesh():
    """torus_mesh(20, 12) with zero-area faces (a repeated vertex) at the front, in a run of three in the middle and at
    the back"""
    m = synth.torus_mesh(20, 12)
    faces = m.faces.copy()
    for f in (0, 1, 200, 201, 202, len(faces) - 1):
        faces[f, 2] = faces[f, 0]
    return m.vs.astype(np.float32), faces


def _mesh(name):
    if name == "one":
        return np.array([[0.5, 0, 0], [2, 0.25, 0], [0, 3, 1]], np.float32), np.array([[0, 1, 2]], np.int64)
    if name == "two":
        return (np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [0, 0, 1], [1, 0, 1], [0, 2, 1]], np.float32),
                np.array([[0, 1, 2], [3, 4, 5]], np.int64))
    if name == "zero_run":
        return _zero_run_mesh()
    m = {"torus": lambda: synth.torus_mesh(20, 12), "sphere": lambda: synth.octahedron_sphere(3),
         "big_torus": lambda: synth.torus_mesh(48, 36)}[name]()                 # big_torus: F = 3456
    return m.vs.astype(np.float32), m.faces


def _equal(dev: torch.Tensor, ref: np.ndarray):
    ref_t = torch.from_numpy(np.ascontiguousarray(ref))
    assert dev.dtype == ref_t.dtype and torch.equal(dev.cpu(), ref_t), (dev.dtype, ref_t.dtype)


def _check_draw(plan, ora, seed, offset, n, order):
    points, face, bary, index = plan.draw(n, seed=seed, offset=offset, order=order)
    ref = ora.draw(seed, offset, n, order)
    _equal(index, ref["index"])
    _equal(face.to(torch.int64), ref["face"])
    _equal(bary, ref["bary"])
    _equal(points, ref["points"])


@pytest.mark.parametrize("name", ["one", "two", "torus", "sphere", "big_torus", "zero_run"])
def test_sampler_equals_the_oracle_bit_for_bit(name):
    vs, faces = _mesh(name)
    ora = SO.SamplerOracle(vs, faces)
    if name == "big_torus":
        assert len(faces) > 3000
    if name == "zero_run":
        assert ora.n_zero_weight == 6 and ora.w[0] == 0 and ora.w[-1] == 0 and not ora.w[200:203].any()
    with capi.SamplerPlan(_t(vs), _t(faces, torch.int64)) as plan:
        assert (plan.total_weight, plan.scale_exponent, plan.n_zero_weight) == (ora.W, ora.s, ora.n_zero_weight)
        w, cdf = plan.export()
        _equal(w, ora.w.view(np.int64))
        _equal(cdf, ora.cdf.view(np.int64))
        for order in ("face", "draw"):
            for n in NS:
                _check_draw(plan, ora, SEED_HI, 0, n, order)
            _check_draw(plan, ora, SEED_HI, (1 << 32) - 3, 8, order)           # the carry into the counter's high word
            _check_draw(plan, ora, 7, 0, 65, order)
        assert plan.draw(0)[0].shape == (0, 3)


def test_sample_surface_returns_the_oracles_samples():
    vs, faces = _mesh("two")
    s = evaluate.sample_surface((vs, faces), 3, seed=7, order="draw")
    assert s.face.dtype == torch.int64 and s.face.tolist() == [1, 1, 0] and s.index.tolist() == [0, 1, 2]
    assert s.bary.tolist() == [[13424538, 1915578, 1437100], [2175213, 13894913, 707090], [11011484, 3227012, 2538720]]
    assert s.points[0].double().tolist() == [0.11417734622955322, 0.17131567001342773, 1.0]
    assert s.total_weight == 1 << 31 and s.n_zero_weight == 0
    s = evaluate.sample_surface((vs, faces), 3, seed=7)                         # "face" is the default order
    assert s.index.tolist() == [2, 0, 1] and s.face.tolist() == [0, 1, 1]


def test_locate_at_the_ends_of_every_slot():
    """Random draws do not hit the first and the last offset of a face's slot, nor the slots beside a run of weight 0."""
    vs, faces = _zero_run_mesh()
    ora = SO.SamplerOracle(vs, faces)
    cdf = [int(x) for x in ora.cdf]
    weighted = [f for f in range(len(faces)) if ora.w[f] > 0]
    t = [cdf[f] for f in weighted] + [cdf[f + 1] - 1 for f in weighted] + [0, ora.W - 1]
    want = weighted + weighted + [weighted[0], weighted[-1]]
    assert weighted[0] == 2 and weighted[-1] == len(faces) - 2 and 199 in weighted and 203 in weighted
    with capi.SamplerPlan(_t(vs), _t(faces, torch.int64)) as plan:
        got = plan.locate(torch.tensor(t, dtype=torch.int64, device=DEV))
    assert got.dtype == torch.int32 and got.tolist() == want
    assert want == [ora.locate(x) for x in t]


def _jittered(m, scale=0.05, seed=3):
    return (m.vs + np.random.default_rng(seed).normal(0, scale, m.vs.shape)).astype(np.float32)


@pytest.fixture(scope="module")
def pair():
    """gt = torus_mesh(20, 12); out = the same faces over jittered vertices; one surface_distance result and the float64
    closest-point answers for its points, shared by the tests below and left unchanged"""
    m = synth.torus_mesh(20, 12)
    a = (m.vs.astype(np.float32), m.faces)
    b = (_jittered(m), m.faces)
    n, seed, tau = 200, 5, 0.03
    r = evaluate.surface_distance(a, b, n=n, seed=seed, tau=tau, order="face")
    ref = {}
    for d, src, dst, sd in (("ab", a, b, seed), ("ba", b, a, seed + 1)):
        smp = SO.SamplerOracle(*src).draw(sd, 0, n, "face")
        pts = np.concatenate([smp["points"], src[0]])
        ora = MO.SurfaceOracle(*dst)
        ref[d] = {"samples": smp, "points": pts, "query": ora.query(pts), "l_max": ora.l_max}
    return {"a": a, "b": b, "n": n, "seed": seed, "tau": tau, "r": r, "ref": ref}


def test_surface_distance_is_reproducible(pair):
    r2 = evaluate.surface_distance(pair["a"], pair["b"], n=pair["n"], seed=pair["seed"], tau=pair["tau"], order="face")
    r1 = pair["r"]
    assert set(r1) == {"ab", "ba", "hausdorff", "chamfer", "diag", "hausdorff_rel", "chamfer_rel", "normal_consistency"}
    for k in r1:
        if k in ("ab", "ba"):
            assert set(r1[k]) == {"max", "mean", "rms", "n", "within", "normal_consistency", "points", "dist", "face_from",
                                  "face_to", "closest"}
            for kk, v in r1[k].items():
                if isinstance(v, torch.Tensor):
                    assert v.dtype == r2[k][kk].dtype and torch.equal(v, r2[k][kk]), (k, kk)
                else:
                    assert v == r2[k][kk], (k, kk)
        else:
            assert r1[k] == r2[k], k


@pytest.mark.parametrize("order", ["draw", "face"])
def test_chunks_of_a_stream_concatenate(order):
    vs, faces = _mesh("sphere")
    whole = evaluate.sample_surface((vs, faces), 300, seed=SEED_HI, order=order)
    parts = [evaluate.sample_surface((vs, faces), 100, seed=SEED_HI, offset=o, order=order) for o in (0, 100, 200)]
    cat = [torch.cat([getattr(p, k) for p in parts]) for k in ("points", "face", "bary", "index")]
    want = [whole.points, whole.face, whole.bary, whole.index]
    if order == "face":                     # equal as sets: sort both by the draw index
        assert not torch.equal(cat[3], want[3])
        pc, pw = torch.argsort(cat[3]), torch.argsort(want[3])
        cat, want = [x[pc] for x in cat], [x[pw] for x in want]
    assert want[3].tolist() == list(range(300))
    for x, y in zip(cat, want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("d", ["ab", "ba"])
def test_distances_against_float64(pair, d):
    """Every device distance within the bound the C ABI states for the query, 1e-5 (dist + longest edge) of the float64
    distance; max / mean / rms within that bound propagated: the largest, the mean and the root mean square of the
    per-point bounds (|max x - max y| <= max |x - y|, the means likewise, and | ||x|| - ||y|| | <= ||x - y||)."""
    res, ref, n = pair["r"][d], pair["ref"][d], pair["n"]
    _equal(res["points"], ref["points"])                       # the device's samples ARE the oracle's
    _equal(res["face_from"][:n], ref["samples"]["face"])
    assert (res["face_from"][n:] == -1).all() and res["face_from"].shape[0] == len(ref["points"])
    d64 = ref["query"]["dist"]
    dev = res["dist"].cpu().numpy().astype(np.float64)
    tol = 1e-5 * (d64 + ref["l_max"])
    err = np.abs(dev - d64)
    print(f"{d}: worst |d - d64| / tol = {(err / tol).max():.3g}")
    assert (dev >= 0).all() and (err <= tol).all(), (err / tol).max()
    N = len(d64)
    slack = 1 + 4 * N * EPS
    assert res["n"] == N
    assert abs(res["max"] - d64.max()) <= tol.max() * slack
    assert abs(res["mean"] - math.fsum(d64.tolist()) / N) <= tol.mean() * slack
    assert abs(res["rms"] - math.sqrt(math.fsum((d64 * d64).tolist()) / N)) <= math.sqrt((tol * tol).mean()) * slack
    clear = ref["query"]["second"] - d64 > tol
    assert (res["face_to"].cpu().numpy()[clear] == ref["query"]["face"][clear]).all()


@pytest.mark.parametrize("d", ["ab", "ba"])
def test_sums_and_counts_are_exact_given_the_distances(pair, d):
    """The float64 sums within N 2^-52 relative of math.fsum over the device's own distances; ``n`` and ``within`` exact."""
    res, tau = pair["r"][d], pair["tau"]
    dist = res["dist"]
    N = dist.shape[0]
    mx, s1, s2, cnt, skipped = capi.distance_stats(dist, tau).tolist()
    wmx, ws1, ws2, wcnt, wskip = SO.distance_stats(dist.cpu().numpy(), tau)
    assert mx == wmx and cnt == wcnt and skipped == wskip == 0 and 0 < cnt < N
    assert abs(s1 - ws1) <= N * EPS * ws1 and abs(s2 - ws2) <= N * EPS * ws2
    assert res["n"] == N and res["within"] == wcnt / N and res["max"] == mx
    assert res["mean"] == s1 / N and res["rms"] == math.sqrt(s2 / N)


@pytest.mark.parametrize("N", [1, 255, 257, 70000, 300001])
def test_distance_stats_sizes_and_skipped_rows(N):
    """One block, a ragged second block, many blocks of one run of 256 each, and (N > 1024 * 256) blocks whose runs are
    longer; infinite rows are skipped and counted."""
    rng = np.random.default_rng(N)
    d = rng.normal(0, 1, N).astype(np.float32)
    d[rng.integers(0, N, max(N // 50, 1))] = np.inf
    d[N // 2] = -np.inf
    tau = 0.5
    got = capi.distance_stats(_t(d), tau).tolist()
    want = SO.distance_stats(d, tau)
    assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4] >= 1
    assert abs(got[1] - want[1]) <= N * EPS * want[1] and abs(got[2] - want[2]) <= N * EPS * want[2]
    assert capi.distance_stats(_t(d)).tolist()[3] == 0                           # no tau: nothing counted
    assert capi.distance_stats(_t(d), tau).tolist() == got                      # a fixed order: the same bits


def test_consistent_with_mesh_distance(pair):
    """With no samples and the vertices appended, direction ab IS the reference's metric: mean / diag = hd_all."""
    a, b = pair["a"], pair["b"]
    r = evaluate.surface_distance(a, b, n=0, vertices=True)
    want = evaluate.mesh_distance(a, a, b)
    N = len(a[0])
    assert r["ab"]["n"] == N and r["ab"]["points"].shape == (N, 3)
    assert abs(r["diag"] - want["diag"]) <= 4 * EPS * want["diag"]
    assert abs(r["ab"]["mean"] / r["diag"] - want["hd_all"]) <= N * EPS * want["hd_all"]
    assert math.isnan(r["ab"]["normal_consistency"]) and math.isnan(r["normal_consistency"])    # no samples, no normals


def test_a_spike_the_one_sided_mean_cannot_see():
    """One vertex of out pushed out along its normal by h = 10 mean edges.  Every gt vertex still has out's surface
    nearby, so hd_all moves by less than h / V / diag; the distance from out to gt sees the whole of h."""
    m = synth.torus_mesh(20, 12, jitter=0.0)
    gt = (m.vs.astype(np.float32), m.faces)
    V = len(gt[0])
    edge = float(np.linalg.norm(m.vs[m.edges[:, 0]] - m.vs[m.edges[:, 1]], axis=1).mean())
    h = 10 * edge
    v = 0                                                   # theta = phi = 0: on the outer equator, normal +x
    assert np.allclose(m.vs[v, 1:], 0) and m.vs[v, 0] == np.abs(m.vs).max()
    out_vs = gt[0].copy()
    out_vs[v, 0] += np.float32(h)
    out = (out_vs, m.faces)
    diag = float(np.linalg.norm(m.vs.max(0) - m.vs.min(0)))
    base = evaluate.mesh_distance(gt, gt, gt)["hd_all"]
    hd_all = evaluate.mesh_distance(gt, gt, out)["hd_all"]
    assert hd_all < base + h / V / diag
    r = evaluate.surface_distance(gt, out, n=500, seed=1)
    assert r["ba"]["max"] >= 0.5 * h
    assert r["hausdorff"] == r["ba"]["max"] > r["ab"]["max"]
    assert r["hausdorff_rel"] == r["hausdorff"] / r["diag"] >= 0.5 * h / diag * (1 - 1e-6)
    assert r["chamfer"] == r["ab"]["mean"] + r["ba"]["mean"] and r["chamfer_rel"] == r["chamfer"] / r["diag"]
    # and without the appended vertices the samples on the spike's cone still see most of it
    assert evaluate.surface_distance(gt, out, n=500, seed=1, vertices=False)["ba"]["max"] >= 0.5 * h


def test_face_mask_confines_the_draws():
    vs, faces = _mesh("torus")
    mask = np.random.default_rng(8).random(len(faces)) < 0.3
    s = evaluate.sample_surface((vs, faces), 500, seed=2, face_mask=mask)
    assert mask[s.face.cpu().numpy()].all() and s.n_zero_weight == int((~mask).sum())
    ref = SO.SamplerOracle(vs, faces, face_mask=mask).draw(2, 0, 500, "face")
    _equal(s.points, ref["points"])
    _equal(s.face, ref["face"])
    r = evaluate.surface_distance((vs, faces), (vs, faces), n=300, a_face_mask=torch.from_numpy(mask).to(DEV), vertices=False)
    assert mask[r["ab"]["face_from"].cpu().numpy()].all() and not mask[r["ba"]["face_from"].cpu().numpy()].all()
    with pytest.raises(ValueError, match="weight 0"):
        evaluate.surface_distance((vs, faces), (vs, faces), n=10, a_face_mask=np.zeros(len(faces), bool))
    with pytest.raises(ValueError, match="weight 0"):
        evaluate.sample_surface((vs, faces), 1, face_mask=np.zeros(len(faces), bool))
    assert evaluate.sample_surface((vs, faces), 0, face_mask=np.zeros(len(faces), bool)).points.shape == (0, 3)


def test_normal_consistency(pair):
    a, b, n = pair["a"], pair["b"], pair["n"]
    for d, src, dst in (("ab", a, b), ("ba", b, a)):
        res = pair["r"][d]
        fa, fb = res["face_from"][:n].to(torch.int32), res["face_to"][:n]
        s, c = capi.normal_agreement(_t(src[0]), _t(src[1], torch.int64), fa, _t(dst[0]), _t(dst[1], torch.int64), fb).tolist()
        ws, wc = SO.normal_agreement(src[0], src[1], fa.cpu().numpy(), dst[0], dst[1], fb.cpu().numpy())
        assert c == wc == n and abs(s - ws) <= n * EPS * ws
        assert res["normal_consistency"] == s / c and 0.5 < s / c <= 1.0
    assert pair["r"]["normal_consistency"] == 0.5 * (pair["r"]["ab"]["normal_consistency"] + pair["r"]["ba"]["normal_consistency"])
    # skipped pairs: a negative id, "no face", a zero normal on either side
    vs, faces = _zero_run_mesh()
    fa = torch.tensor([5, -1, 7, 0, 9, 300], dtype=torch.int32, device=DEV)
    fb = torch.tensor([5, 3, capi.NO_FACE, 4, 201, 300], dtype=torch.int32, device=DEV)
    s, c = capi.normal_agreement(_t(vs), _t(faces, torch.int64), fa, _t(vs), _t(faces, torch.int64), fb).tolist()
    assert c == 2 and abs(s - 2.0) <= 4 * EPS
    assert SO.normal_agreement(vs, faces, fa.cpu().numpy(), vs, faces, fb.cpu().numpy())[1] == 2
    # a mesh against itself, and against its reversed copy: the term is |cos|
    m = synth.octahedron_sphere(3)
    same = evaluate.surface_distance(m, m, n=500, seed=4)["normal_consistency"]
    rev = evaluate.surface_distance(m, (m.vs, m.faces[:, ::-1].copy()), n=500, seed=4)["normal_consistency"]
    assert same > 1 - 1e-6 and rev == same


def test_error_paths():
    vs, faces = _mesh("two")
    with pytest.raises(SemigcnLibraryError, match="HIP device only"):
        evaluate.sample_surface((torch.from_numpy(vs), torch.from_numpy(faces)), 4)
    with pytest.raises(SemigcnLibraryError):
        evaluate.surface_distance((torch.from_numpy(vs), torch.from_numpy(faces)), (vs, faces), n=4)
    bad = vs.copy()
    bad[4, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        evaluate.sample_surface((bad, faces), 4)
    bad[4, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        evaluate.sample_surface((bad, faces), 4)
    for wrong in (len(vs), -1):
        f = faces.copy()
        f[1, 2] = wrong
        with pytest.raises(ValueError, match="outside"):
            evaluate.sample_surface((vs, f), 4)
    with pytest.raises(ValueError, match="order"):
        evaluate.sample_surface((vs, faces), 4, order="morton")
    with pytest.raises(ValueError):
        evaluate.sample_surface((vs, faces), -1)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        evaluate.sample_surface((vs, faces.reshape(-1)), 4)
    # the process stays healthy
    assert evaluate.sample_surface((vs, faces), 3, seed=7, order="draw").face.tolist() == [1, 1, 0]


def test_command_line(tmp_path, capsys):
    m = synth.torus_mesh(20, 12)
    g, o = str(tmp_path / "gt.obj"), str(tmp_path / "out.obj")
    mesh_common.write_obj(g, m.vs.astype(np.float32), m.faces)
    mesh_common.write_obj(o, _jittered(m), m.faces)
    new = {"hausdorff", "chamfer", "hausdorff_rel", "chamfer_rel", "max_ab", "mean_ab", "rms_ab", "max_ba", "mean_ba", "rms_ba",
           "normal_consistency", "sample_ms", "query_ms", "stats_ms"}

    def run(*args):
        assert evaluate.main(["--gt", g, "--out", o, *args]) == 0
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 1
        return json.loads(lines[0])

    plain, plain_org = run(), run("--org", g)
    assert list(plain) == ["hd_all"] and list(plain_org) == ["hd_all", "hd_hole", "n_hole", "diag"]
    r = run("--sampled", "2000")
    assert set(r) == {"hd_all"} | new and r["hd_all"] == plain["hd_all"]
    assert r["hausdorff"] == max(r["max_ab"], r["max_ba"]) > 0 and r["chamfer"] == r["mean_ab"] + r["mean_ba"]
    assert all(r[k] >= 0 for k in ("sample_ms", "query_ms", "stats_ms"))
    r2 = run("--sampled", "2000", "--org", g, "--seed", "3", "--tau", "0.05", "--order", "draw")
    assert set(r2) == set(plain_org) | new | {"within_ab", "within_ba"} and 0 < r2["within_ab"] <= 1
    want = evaluate.surface_distance(mesh_common.read_obj(g), mesh_common.read_obj(o), n=2000, seed=3, tau=0.05, order="draw")
    assert r2["hausdorff"] == want["hausdorff"] and r2["chamfer"] == want["chamfer"]
    assert r2["normal_consistency"] == want["normal_consistency"]
