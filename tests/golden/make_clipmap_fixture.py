#!/usr/bin/env python3
"""Generates tests/golden/clipmap_low_inner.npz from the reference's water mesh (assets/water/clipmap_low.obj): the vertices and the
fan-triangulated faces inside max(|x|, |z|) <= 128 m.  Run where the reference checkout exists:
    python tests/golden/make_clipmap_fixture.py path/to/assets/water/clipmap_low.obj
The file's faces are 4-, 5- and 7-gons at the ring transitions; each is fanned from its first vertex (a zero-area triangle at a
T-junction is kept: it is legitimate input).  A triangle is kept when all three of its vertices are inside the square; the indices are
remapped to the vertices that remain.  The fixture is data (positions and index triples); tests/test_mesh_draw.py reads it, no test
reads the reference checkout."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 128.0


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    path = sys.argv[1]
    verts, tris, sides = [], [], {}
    for line in open(path):
        w = line.split()
        if not w:
            continue
        if w[0] == "v":
            verts.append([float(v) for v in w[1:4]])
        elif w[0] == "f":
            idx = [int(v.split("/")[0]) for v in w[1:]]
            idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
            sides[len(idx)] = sides.get(len(idx), 0) + 1
            for k in range(1, len(idx) - 1):
                tris.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, np.float32)
    t = np.asarray(tris, np.int64)
    inside = np.abs(v[:, [0, 2]]).max(axis=1) <= LIMIT
    keep = inside[t].all(axis=1)
    t = t[keep]
    used = np.unique(t)
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    out_v = v[used]
    out_t = remap[t].astype(np.int32)
    e1, e2 = out_v[out_t[:, 1]] - out_v[out_t[:, 0]], out_v[out_t[:, 2]] - out_v[out_t[:, 0]]
    ny = np.cross(e1.astype(np.float64), e2.astype(np.float64))[:, 1]
    print(f"{path}: {len(v)} vertices, faces by side count {sides}; kept {len(out_v)} vertices, {len(out_t)} triangles "
          f"({(ny == 0).sum()} of zero area, {(ny > 0).sum()} with (v1 - v0) x (v2 - v0) up, {(ny < 0).sum()} down), "
          f"y range {out_v[:, 1].min()} .. {out_v[:, 1].max()}")
    dst = os.path.join(HERE, "clipmap_low_inner.npz")
    np.savez_compressed(dst, vertices=out_v, triangles=out_t)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
