"""Writes tests/golden/g8_vertex_update.npz: the reference's own ``Models.vertex_updating(pos, new_fn, mesh, loop)``
(util/models.py:239-252), run unchanged through ``oracle.ref_shim.load()``, for ``loop`` 1 and 10 on the ``sphere`` and
``open`` meshes of tests/golden/g6_bnf.npz.  The file holds only the recorded results; the inputs (``pos``, ``new_fn``,
``faces``) are read from g6 and not duplicated.  The mesh object handed to the reference carries what the function reads:
``.faces`` and ``.vf`` (per vertex, the set of faces that name it, as util/mesh.py:191-197 builds it).

    python tools/make_golden_denoise.py          # needs the reference tree (oracle.ref_shim.available())
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

MESHES, LOOPS = ("sphere", "open"), (1, 10)


def mesh_for(faces: np.ndarray, num_vertices: int):
    vf = [set() for _ in range(num_vertices)]
    for i, f in enumerate(faces.tolist()):
        for v in f:
            vf[v].add(i)
    return types.SimpleNamespace(faces=faces, vf=vf)


def reference_results(g6):
    """{"<mesh>/loop<k>": float32 [V, 3]} from the reference."""
    ref = ref_shim.load()
    out = {}
    for name in MESHES:
        faces, pos, fn = g6[f"{name}/faces"], g6[f"{name}/pos"], g6[f"{name}/new_fn"]
        mesh = mesh_for(faces, pos.shape[0])
        for loop in LOOPS:
            got = ref.models.vertex_updating(torch.from_numpy(pos), torch.from_numpy(fn), mesh, loop=loop)
            out[f"{name}/loop{loop}"] = got.numpy().astype(np.float32)
    return out


def main() -> int:
    if not ref_shim.available():
        print("the reference tree is not available", file=sys.stderr)
        return 1
    g6 = np.load(os.path.join(ROOT, "tests", "golden", "g6_bnf.npz"))
    path = os.path.join(ROOT, "tests", "golden", "g8_vertex_update.npz")
    np.savez_compressed(path, **reference_results(g6))
    print(path, os.path.getsize(path), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
