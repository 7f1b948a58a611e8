"""FP64 twin of a mesh draw (include/ocean_waves.h ow_mesh_draw), written from the definition and not from csrc/ow_mesh.h: brute-force
Moeller-Trumbore of every pixel's ray against every triangle of the FP32 vertex records, the nearest view depth inside (near, far]
per pixel, barycentrics in space (which is the perspective-correct interpolation) and the varyings.  Test infrastructure
(tests/test_mesh_draw.py)."""
import numpy as np

import render_twin as RT


def draw(vertices, triangles, cam_position, cam_basis, fov_y_degrees, width, height, near, far, cull_back=False):
    """vertices: MESH_VERTEX records (position, uv, wave_height, flags read); triangles [T][3].  Returns a dict of [H][W] arrays:
    hit, tri (-1 without a hit), below (seen from the underside), depth (view depth), t (along the unit ray), position [3], uv [2],
    wave_height, view_position [3], min_bary (the smallest barycentric of the drawn triangle) and gap (how much deeper, in metres of view
    depth, the next-nearest other triangle's hit is; inf without one)."""
    P = np.asarray(vertices["position"], np.float64)
    ok = np.asarray(vertices["flags"]) == 0
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    usable = ok[tri].all(axis=1)
    o = np.asarray(cam_position, np.float64)
    B = np.asarray(cam_basis, np.float64).reshape(3, 3)
    fwd = -B[:, 2]
    dirs = RT.pixel_directions(cam_basis, fov_y_degrees, width, height).reshape(-1, 3)
    v0, v1, v2 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    normal = np.cross(e1, e2)
    npix, ntri = len(dirs), len(tri)
    out = dict(hit=np.zeros(npix, bool), tri=np.full(npix, -1, np.int64), below=np.zeros(npix, bool), depth=np.zeros(npix), t=np.zeros(npix),
               position=np.zeros((npix, 3)), uv=np.zeros((npix, 2)), wave_height=np.zeros(npix), view_position=np.zeros((npix, 3)),
               min_bary=np.zeros(npix), gap=np.full(npix, np.inf))
    tvec = o[None, :] - v0                               # [T][3]
    qvec = np.cross(tvec, e1)                            # [T][3]
    chunk = max(1, 2_000_000 // max(ntri, 1))
    for lo in range(0, npix, chunk):
        d = dirs[lo:lo + chunk]                          # [p][3]
        pvec = np.cross(d[:, None, :], e2[None, :, :])   # [p][T][3]
        det = np.einsum("tk,ptk->pt", e1, pvec)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u = np.einsum("tk,ptk->pt", tvec, pvec) * inv
            v = np.einsum("pk,tk->pt", d, qvec) * inv
            t = np.einsum("tk,tk->t", e2, qvec)[None, :] * inv
        depth = t * (d @ fwd)[:, None]
        facing_up = np.einsum("pk,tk->pt", d, normal) < 0        # the ray runs against the normal: the upper side is seen
        good = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (depth > near) & (depth <= far) & usable[None, :]
        if cull_back:
            good &= facing_up
        dd = np.where(good, depth, np.inf)
        best = dd.argmin(axis=1)
        rows = np.arange(len(d))
        hit = np.isfinite(dd[rows, best])
        other = dd.copy()
        other[rows, best] = np.inf
        sl = slice(lo, lo + len(d))
        out["hit"][sl] = hit
        out["tri"][sl] = np.where(hit, best, -1)
        with np.errstate(invalid="ignore"):
            out["gap"][sl] = other.min(axis=1) - dd[rows, best]
        ub, vb = u[rows, best], v[rows, best]
        w = np.stack([1.0 - ub - vb, ub, vb], axis=1)
        out["min_bary"][sl] = w.min(axis=1)
        out["below"][sl] = ~facing_up[rows, best]
        out["depth"][sl] = depth[rows, best]
        out["t"][sl] = t[rows, best]
        idx = tri[best]                                   # [p][3]
        for name, src in (("position", P), ("uv", np.asarray(vertices["uv"], np.float64)),
                          ("view_position", np.asarray(vertices["view_position"], np.float64))):
            out[name][sl] = np.einsum("pc,pck->pk", w, src[idx])
        out["wave_height"][sl] = np.einsum("pc,pc->p", w, np.asarray(vertices["wave_height"], np.float64)[idx])
    miss = ~out["hit"]
    out["gap"][miss] = np.inf
    for k, a in out.items():
        if k not in ("hit", "tri", "gap"):
            a[miss] = 0
    return {k: a.reshape((height, width) + a.shape[1:]) for k, a in out.items()}
