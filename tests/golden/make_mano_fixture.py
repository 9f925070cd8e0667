#!/usr/bin/env python
"""Generate tests/golden/mano_subdivide_fixture.npz by running the REFERENCE's own mis_utils.edge_subdivide (the function the dataset
applies three times to each posed hand, dataset_one_shot.py:299-325) on a 4 x 5 grid mesh and on the same mesh with every face turned
over (faces[:, [0, 2, 1]]: the mirrored hand's winding, which changes the order edges first appear in).

Runs only where the reference tree is present; the resulting .npz is data (inputs and recorded outputs, a few thousand numbers) and
is committed; nothing of the reference travels. mis_utils imports openmesh further down, which is not installed: under the stub
modules of make_host_fixtures.py (openmesh added to its list here) the file imports and the function runs.

    vertices                         (20, 3) float32, faces (24, 3) int64: the input mesh ("a"); faces_b the turned-over faces ("b")
    {a,b}_l{1,2,3}_vertices          float32: the function's vertices after that many applications (it computes them in float64)
    {a,b}_l{1,2,3}_faces, _edges     int64

Usage: python tests/golden/make_mano_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mano_subdivide_fixture.npz")
NX, NY, SEED = 4, 5, 3


def grid_mesh(nx, ny, seed):
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v = np.stack([ii.reshape(-1) / (nx - 1.0), jj.reshape(-1) / (ny - 1.0), np.zeros(nx * ny)], 1) + 0.05 * rng.randn(nx * ny, 3)
    q = (ii[:-1, :-1] * ny + jj[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([q, q + ny, q + 1], 1), np.stack([q + 1, q + ny, q + ny + 1], 1)])
    return v.astype(np.float32), f.astype(np.int64)


def main():
    host._StubFinder.ROOTS = host._StubFinder.ROOTS + ("openmesh",)
    host.install_stubs([])
    sys.path.insert(0, REF)
    import mis_utils

    v0, f0 = grid_mesh(NX, NY, SEED)
    out = {"vertices": v0, "faces": f0, "faces_b": f0[:, [0, 2, 1]].copy()}
    for tag, faces in (("a", f0), ("b", out["faces_b"])):
        v, f = v0.astype(np.float64), faces
        for level in (1, 2, 3):
            v, f, e = mis_utils.edge_subdivide(v, f)
            f = np.asarray(f).astype(np.int64)
            out[f"{tag}_l{level}_vertices"] = np.asarray(v).astype(np.float32)
            out[f"{tag}_l{level}_faces"] = f
            out[f"{tag}_l{level}_edges"] = np.asarray(e).astype(np.int64)
    assert not np.array_equal(out["a_l1_edges"], out["b_l1_edges"])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
