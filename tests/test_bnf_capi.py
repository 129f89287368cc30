"""The bilateral face-normal filter below the C ABI (csrc/mesh_bnf.hip), without a device: the entry points exist in the
header, the ctypes table and the library; they reject bad arguments before touching a device; the Python operations
have no CPU path; and train.fn_bnf_detach_loss -- the drop-in with the reference's signature -- reproduces golden g6."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import golden_util as GU
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_bnf_blocks", "sg_bnf_scratch_bytes", "sg_bnf_filter", "sg_mesh_loss_cad_finalize", "sg_mesh_loss_cad_bwd_det")


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    # the entries they extend keep their ABI-version-1 signatures
    assert len(capi._SIGNATURES["sg_mesh_loss_finalize"][1]) == 8 and len(capi._SIGNATURES["sg_mesh_loss_bwd_det"][1]) == 14
    assert capi.load().sg_abi_version() == 1


def test_sizing_rules():
    lib = capi.load()
    assert lib.sg_bnf_blocks(0) == 1 and lib.sg_bnf_blocks(256) == 1 and lib.sg_bnf_blocks(257) == 2
    assert lib.sg_bnf_blocks(-1) == -1 and lib.sg_bnf_scratch_bytes(-1) == -1
    for F in (1, 255, 1000, 2_000_000):
        nb = lib.sg_bnf_blocks(F)
        assert lib.sg_bnf_scratch_bytes(F) >= 5 * 16 * F + 4 * nb + 8 and lib.sg_bnf_scratch_bytes(F) % 16 == 0


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_float * 68)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    ok = dict(pos=p, faces=p, f2f=p, V=4, F=2, loop=5, sigma=0.3, start=None, fn=p, nf=ctypes.c_void_p(p.value + 64), part=None,
              scratch=ctypes.c_void_p(p.value + 128), stream=None)

    def filt(**kw):
        a = dict(ok, **kw)
        return lib.sg_bnf_filter(a["pos"], a["faces"], a["f2f"], a["V"], a["F"], a["loop"], a["sigma"], a["start"], a["fn"], a["nf"],
                                 a["part"], a["scratch"], a["stream"])
    assert filt(F=-1) == -1 and b"negative" in lib.sg_last_error()
    assert filt(V=-1) == -1
    assert filt(loop=-1) == -1 and b"loop" in lib.sg_last_error()
    assert filt(sigma=0.0) == -1 and b"sigma_s" in lib.sg_last_error()
    assert filt(sigma=-0.3) == -1
    for name in ("pos", "faces", "f2f", "fn", "nf", "scratch"):
        assert filt(**{name: None}) == -1 and b"null pointer" in lib.sg_last_error(), name
    assert filt(nf=p) == -1 and b"distinct" in lib.sg_last_error()
    assert filt(scratch=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.sg_last_error()

    fin = lib.sg_mesh_loss_cad_finalize
    assert fin(None, 0, 1.0, 0.0, 1.0, 0.0, None, 1, 10, 4.0, p, None) == -1 and b"bad argument" in lib.sg_last_error()
    assert fin(None, 0, 1.0, 0.0, 1.0, 0.0, p, 1, 10, 4.0, None, None) == -1
    assert fin(None, 0, 1.0, 0.0, 1.0, 0.0, p, 0, 10, 4.0, p, None) == -1
    assert fin(None, 0, 1.0, 0.0, 1.0, 0.0, p, 1, 0, 4.0, p, None) == -1
    assert fin(p, -1, 1.0, 0.0, 1.0, 0.0, p, 1, 10, 4.0, p, None) == -1
    assert fin(p, 1, 0.0, 0.0, 1.0, 0.0, p, 1, 10, 4.0, p, None) == -1       # n_v must be positive, as in sg_mesh_loss_finalize

    bwd = lib.sg_mesh_loss_cad_bwd_det
    assert bwd(p, p, None, None, None, None, p, p, p, 0, 4, -1, None, p, p, None) == -1 and b"bad argument" in lib.sg_last_error()
    assert bwd(p, p, None, None, None, None, p, p, None, 0, 4, 2, None, p, p, None) == -1            # null g
    assert bwd(p, p, None, None, None, None, None, p, p, 0, 4, 2, None, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert bwd(p, p, None, None, None, None, p, None, p, 0, 4, 2, None, p, p, None) == -1            # null n_filtered
    assert bwd(p, p, None, None, p, None, p, p, p, 0, 4, 2, None, p, p, None) == -1                  # target_fn without f_keep
    assert bwd(p, p, None, None, None, None, p, p, p, 0, 4, 2, None, p, p, None) == -1 and b"incidence" in lib.sg_last_error()


def test_python_operations_have_no_cpu_path():
    from semigcn_amd import functional as F_sg
    g = GU.load("g6_bnf.npz")
    pos = torch.from_numpy(g["sphere/pos"])
    faces, f2f = torch.from_numpy(g["sphere/faces"]), torch.from_numpy(g["sphere/f2f"])
    with pytest.raises(capi.SemigcnLibraryError, match="HIP device only"):
        F_sg.bilateral_normal_filter(pos, faces, f2f)
    with pytest.raises(capi.SemigcnLibraryError, match="HIP device only"):
        F_sg.bilateral_normal_loss(pos, faces, f2f)
    with pytest.raises(ValueError, match="f2f"):
        F_sg.mesh_loss(pos, faces, pos, torch.ones(pos.shape[0]), pos[: faces.shape[0]], torch.ones(faces.shape[0]), 1.0, 1.0,
                       1.0, 4.0, k2=4.0)


@pytest.mark.parametrize("name", ["sphere", "open"])
@pytest.mark.parametrize("as_numpy", [True, False])
def test_fn_bnf_detach_loss_vs_reference_golden(name, as_numpy):
    """The drop-in called the way the reference scripts call it (sgcn.py:133-135: positions, their face normals, a mesh
    object with .faces / .f2f) at the bounds of test_host_logic.py::test_bilateral_normal_loss_vs_reference_golden."""
    from semigcn_amd import train
    g = GU.load("g6_bnf.npz")
    pos = torch.from_numpy(g[f"{name}/pos"]).requires_grad_(True)
    faces, f2f = g[f"{name}/faces"], g[f"{name}/f2f"]
    mesh = types.SimpleNamespace(faces=faces if as_numpy else torch.from_numpy(faces), f2f=f2f if as_numpy else torch.from_numpy(f2f))
    fn = train.face_normals(pos, torch.from_numpy(faces))
    loss, new_fn = train.fn_bnf_detach_loss(pos, fn, mesh)
    loss.backward()
    assert abs(float(loss.detach()) - float(g[f"{name}/loss"])) < 1e-6 * float(g[f"{name}/loss"])
    assert np.abs(new_fn.numpy() - g[f"{name}/new_fn"]).max() < 1e-6 and not new_fn.requires_grad
    assert rel(pos.grad, g[f"{name}/dpos"]) < 1e-5
    if name == "open":
        assert (f2f < 0).sum() > 0
    # explicit arguments of the reference's signature; a numpy `pos` is taken as it is (util/loss.py:199-200)
    loss2, _ = train.fn_bnf_detach_loss(g[f"{name}/pos"], fn.detach(), mesh, "l1mae", 5)
    assert float(loss2) == float(loss.detach())


def test_fn_bnf_detach_loss_rejects_other_ltypes():
    from semigcn_amd import train
    mesh = types.SimpleNamespace(faces=np.zeros((1, 3), np.int64), f2f=-np.ones((1, 3), np.int64))
    for ltype in ("mae", "rmse", "l1rmse", "huber"):
        with pytest.raises(NotImplementedError, match="l1mae"):
            train.fn_bnf_detach_loss(torch.zeros(3, 3), torch.zeros(1, 3), mesh, ltype=ltype)
