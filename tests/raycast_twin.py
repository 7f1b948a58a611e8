"""FP64 NumPy twin of the ray cast (include/ocean_waves.h ow_raycast_surface; godotoceanwaves_amd/csrc/ow_raycast.h), built on
query_twin.py: the height field h(x, z) = f(p) D_y(p) with p solving p + f(p) D_xz(p) = (x, z), all in FP64 over the FP16 maps.  Each ray is
sampled densely (at a sixteenth of the device's spacing) from t_in, the height solve warm-started from the previous sample's p moved with
the ray (damped Newton, Jacobian by central differences), and the first sign change of g = y - (water_level + h) is bisected.  On a
folded crest the warm start follows one sheet of the fold; the device's cold solve may pick another.  Test infrastructure."""
import numpy as np

import query_twin as T


class Field:
    def __init__(self, disp, scales, center=None):
        self.d = T.as_f64(disp)
        self.sc = np.asarray(scales, np.float64)
        self.center = center

    def disp(self, p):
        import consumer as K
        return K.displacement_at([self.d[i] for i in range(len(self.sc))], self.sc, p[:, 0], p[:, 1])

    def forward(self, p):
        """(x, z) where the vertex that starts at p is drawn, and its height"""
        f = T.falloff(p, self.center)
        d = self.disp(p)
        return p + f[:, None] * d[:, [0, 2]], f * d[:, 1]

    def solve(self, q, p, iterations=3, h=1e-5, tol=1e-6):
        """p with p + f D_xz(p) = q: damped Newton from p (a step is halved until |F| decreases; where it never does, or det J is
        small, the fixed-point step -F), then, where that left |F| above tol, again from p = q with more iterations.
        Returns (p, height, |F|)."""
        p, r = self._newton(q, p, iterations, h)
        redo = r > tol
        if redo.any():
            p2, r2 = self._newton(q[redo], q[redo].copy(), 20, h)
            better = r2 < r[redo]
            idx = np.nonzero(redo)[0][better]
            p[idx], r[idx] = p2[better], r2[better]
        _, hgt = self.forward(p)
        return p, hgt, r

    def _residual(self, q, p):
        Fq, _ = self.forward(p)
        return Fq - q

    def _newton(self, q, p, iterations, h):
        p = p.copy()
        F = self._residual(q, p)
        r = np.hypot(*F.T)
        for _ in range(iterations):
            live = r > 1e-12
            if not live.any():
                break
            fx = self._residual(q, p + [h, 0.0]) - F
            fz = self._residual(q, p + [0.0, h]) - F
            J = np.stack([fx / h, fz / h], axis=2)   # J[:, k, j] = dF_k / dp_j
            det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
            ok = det > 0.1
            step = -F.copy()
            step[ok, 0] = -(J[ok, 1, 1] * F[ok, 0] - J[ok, 0, 1] * F[ok, 1]) / det[ok]
            step[ok, 1] = -(-J[ok, 1, 0] * F[ok, 0] + J[ok, 0, 0] * F[ok, 1]) / det[ok]
            moved = np.zeros(len(p), bool)
            lam = 1.0
            for _ in range(8):
                todo = live & ~moved
                if not todo.any():
                    break
                pn = p[todo] + lam * step[todo]
                Fn = self._residual(q[todo], pn)
                rn = np.hypot(*Fn.T)
                acc = rn < r[todo]
                ids = np.nonzero(todo)[0][acc]
                p[ids], F[ids], r[ids] = pn[acc], Fn[acc], rn[acc]
                moved[ids] = True
                lam *= 0.5
        return p, r


def raycast(field, o, d, t_in, t_end, spacing, water_level=0.0, bisections=40):
    """o, d [R][3] (d unit), t_in, t_end [R]: the first t in [t_in, t_end] where the class of g changes from its class at t_in, or NaN.
    Sampling step spacing (FP64)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    R = len(o)
    t_hit = np.full(R, np.nan)
    t = np.asarray(t_in, np.float64).copy()
    q = o[:, [0, 2]] + t[:, None] * d[:, [0, 2]]
    p, h, _ = field.solve(q, q.copy(), iterations=12)
    g = o[:, 1] + t * d[:, 1] - (water_level + h)
    above0 = g > 0
    active = np.arange(R)[t < t_end]
    prev_t, prev_p = t.copy(), p.copy()
    brackets = []
    while len(active):
        tn = np.minimum(prev_t[active] + spacing, t_end[active])
        qn = o[active][:, [0, 2]] + tn[:, None] * d[active][:, [0, 2]]
        qp = o[active][:, [0, 2]] + prev_t[active][:, None] * d[active][:, [0, 2]]
        pn, hn, _ = field.solve(qn, prev_p[active] + (qn - qp), iterations=2)
        gn = o[active, 1] + tn * d[active, 1] - (water_level + hn)
        changed = (gn > 0) != above0[active]
        for i in np.nonzero(changed)[0]:
            brackets.append((active[i], prev_t[active[i]], tn[i], prev_p[active[i]].copy()))
        prev_t[active] = tn
        prev_p[active] = pn
        active = active[~changed & (tn < t_end[active])]
    if not brackets:
        return t_hit
    idx = np.array([b[0] for b in brackets])
    a = np.array([b[1] for b in brackets])
    b = np.array([b[2] for b in brackets])
    pa = np.array([b[3] for b in brackets])
    for _ in range(bisections):
        m = 0.5 * (a + b)
        qm = o[idx][:, [0, 2]] + m[:, None] * d[idx][:, [0, 2]]
        qa = o[idx][:, [0, 2]] + a[:, None] * d[idx][:, [0, 2]]
        pm, hm, _ = field.solve(qm, pa + (qm - qa), iterations=3)
        gm = o[idx, 1] + m * d[idx, 1] - (water_level + hm)
        same = (gm > 0) == above0[idx]
        a = np.where(same, m, a)
        pa = np.where(same[:, None], pm, pa)
        b = np.where(same, b, m)
    t_hit[idx] = 0.5 * (a + b)
    return t_hit
