#!/usr/bin/env python
"""Generate tests/golden/uvd_hand_fixture.npz: the UV-topology hand template the UV search (guassianhand_amd/uvd.py) is tested on.

Runs only where the reference tree is present and reads its DATA only — `mano_uv/original mano template/hand.obj` (778 vertices,
1,538 faces, 905 UV vertices), `mano_uv/change/change_r.npy` (the template vertex behind every UV vertex, dataset_one_shot.py:410-419)
and `mano_uv/change/vt.npy` (the (1810, 2) UV table of both hands, dataset_one_shot.py:601-605). The .npz is data and is committed;
nothing of the reference's program text travels.

    verts     (905, 3) float32    the UV-topology vertex positions, verts[change_r]
    faces     (1538, 3) int16     the UV faces (the OBJ's vt indices, zero-based)
    uv_table  (1810, 2) float32   vt.npy: rows 0..904 serve one hand, rows 905..1809 the other

The script ASSERTS (exit status non-zero otherwise) that the OBJ's v / vt face corners and verts[change_r][faces] coincide exactly, that
the table is the OBJ's own 905 vt rows (u / 2, (1 - v) / 2) followed by the same rows shifted by 0.5 in u, and that no face of the
template is near the kernel's zero-area rule (sin^2 of the angle at its first corner above 2^-10).

Usage: python tests/golden/make_uvd_fixture.py <reference directory>      (or GH_REFERENCE=<reference directory>)
"""
import os
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GH_REFERENCE", "")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "uvd_hand_fixture.npz")


def main():
    assert os.path.isdir(os.path.join(REF, "mano_uv")), "pass the reference directory (or set GH_REFERENCE)"
    v, vt, fv, ft = [], [], [], []
    for line in open(os.path.join(REF, "mano_uv", "original mano template", "hand.obj")):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:4]])
        elif tok[0] == "vt":
            vt.append([float(x) for x in tok[1:3]])
        elif tok[0] == "f":
            corners = [c.split("/") for c in tok[1:]]
            assert len(corners) == 3
            fv.append([int(c[0]) - 1 for c in corners])
            ft.append([int(c[1]) - 1 for c in corners])
    v, vt, fv, ft = np.array(v), np.array(vt), np.array(fv), np.array(ft)
    assert v.shape == (778, 3) and vt.shape == (905, 2) and fv.shape == ft.shape == (1538, 3)
    change_r = np.load(os.path.join(REF, "mano_uv", "change", "change_r.npy")).astype(np.int64)
    table = np.load(os.path.join(REF, "mano_uv", "change", "vt.npy"))
    assert change_r.shape == (905,) and table.shape == (1810, 2)
    verts = v[change_r]
    assert np.array_equal(verts[ft], v[fv]), "the OBJ's v / vt corners and verts[change_r][ft] differ"
    half = np.stack([vt[:, 0] / 2, (1 - vt[:, 1]) / 2], 1)         # dataset_one_shot.py:141-147: both hands share one map, side by side
    assert np.allclose(table[:905], half, atol=1e-9) and np.allclose(table[905:], half + [0.5, 0.0], atol=1e-9), "vt.npy is not the OBJ's vt rows"
    assert ft.min() == 0 and ft.max() == 904
    a, b, c = (verts[ft[:, k]] for k in range(3))
    d00, d01, d11 = ((b - a) ** 2).sum(1), ((b - a) * (c - a)).sum(1), ((c - a) ** 2).sum(1)
    sin2 = (d00 * d11 - d01 ** 2) / (d00 * d11)
    assert sin2.min() > 2.0 ** -10, sin2.min()
    np.savez_compressed(OUT, verts=verts.astype(np.float32), faces=ft.astype(np.int16), uv_table=table.astype(np.float32))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; smallest sin^2 at a first corner {sin2.min():.3g}")


if __name__ == "__main__":
    main()
