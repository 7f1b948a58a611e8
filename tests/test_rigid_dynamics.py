"""The floating bodies' integrator (godotoceanwaves_amd/csrc/ow_rigid.h, rigid_integrate and rigid_pose) held to references that do not
share its code: tests/rigid_twin.py (one substep in exact rationals, written from the header's comment) and closed forms.

CPU (the header as plain C++, tests/bodies/bodies_harness.cpp): random single substeps and pose records against the twin; the basis by hand
at q = (1/2, 1/2, 1/2, 1/2); spherical inertia under a constant torque; a torque-free spin of 1000 substeps against the rotation it must be;
a tilted box righting itself on a calm sea; pose records saturating at +-FLT_MAX.  GPU (fused and split kernels, 256^2 x 2, seven bodies in
two blocks): every single substep, in the air and on the water, against the twin's step from the previous device state and the record read
back; the closed forms through ow_bodies_create / ow_bodies_step / ow_bodies_get_state.

Every tolerance is the twin's C u magnitude (the rounding counts stand in rigid_twin.py) or is derived in the test's docstring.  The tests
print the worst ratio error / (u magnitude) per component; profiles/rigid_twin_margins.txt records them."""
from fractions import Fraction

import numpy as np
import pytest

from godotoceanwaves_amd import _lib
from godotoceanwaves_amd.presets import cascade_preset, UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import rigid_twin as T
from cpu_builds import CpuSet
from cpu_builds import bodies_harness as harness  # noqa: F401 (fixture)
from scenes import (airborne_bodies, BASIS_IINV, BASIS_TORQUE, basis_bodies, calm, crate, device_read, make_bodies, quaternion, random_rigid_states,
                    saturated_bodies, scales_of, seven_bodies, SPIN_Q0, SPIN_W, spin_bodies, tilted_box)

G32 = float(np.float32(9.81))      # the gravity the integrator uses: the FP32 default of ow_buoyancy_options, widened
FLT_MAX = float(np.finfo(np.float32).max)
MAX_SUBSTEPS = _lib.OW_BODIES_MAX_SUBSTEPS
MOVED = ("position", "orientation", "linear_velocity", "angular_velocity")


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------

def finish(L, state, result, dt, flag=0):
    """harness_rigid_finish on a copy of one state record: (the new record, the new flag)"""
    s = np.array(state, W.RIGID_BODY).reshape(1).copy()
    r = np.array(result, W.BUOYANCY_RESULT).reshape(1).copy()
    f = np.array([flag], np.int32)
    L.harness_rigid_finish(s.ctypes.data, f.ctypes.data, r.ctypes.data, float(dt), G32)
    return s[0], int(f[0])


def hold_step(before, record, after, dt, worst, what, flag=0):
    """`after` must be the twin's step of `before` from `record` within C u magnitude on every component (exactly, in rationals), and every
    field a substep does not move must be `before`'s byte for byte; a body the twin does not integrate must come back whole.  worst: the
    largest ratios seen, updated"""
    stepped = T.step(before, record, dt, G32, flag)
    if stepped is None:
        assert after.tobytes() == before.tobytes(), (what, "a body that is not integrated moved")
        return False
    assert stepped["finite"], what
    for name, field in T.FIELD.items():
        for k, (got, (want, mag)) in enumerate(zip(T.exact(after[field]), stepped[name])):
            assert abs(got - want) <= T.C[name] * T.U * mag, (what, name, k, float(abs(got - want) / (T.U * mag)) if mag else "magnitude 0")
    rest = np.array(before, W.RIGID_BODY).reshape(1).copy()
    for field in MOVED:
        rest[field][0] = after[field]
    assert rest[0].tobytes() == after.tobytes(), (what, "a field outside o, q, v, w changed")
    for name, r in T.ratios(after, stepped).items():
        worst[name] = max(worst.get(name, 0.0), r)
    worst["condition"] = max(worst.get("condition", 1.0), float(stepped["condition"]))
    return True


def report(title, worst):
    print(f"{title}: worst error / (u magnitude): " + ", ".join(f"{k} {worst[k]:.2f} (C {T.C[k]})" for k in ("v", "w", "o", "q") if k in worst)
          + f"; largest condition of the normalisation {worst.get('condition', 1.0):.6f}")


def hold_pose(record, state, what):
    """a pose record against the twin's: o, v and w the saturated narrowing bit for bit, R within one FP32 rounding of the header's FP64 R,
    which is within C_R u magnitude of the exact one"""
    p = T.pose(state)
    assert p["ok"], what
    assert record["transform"][9:].tobytes() == p["o32"].tobytes(), what
    assert record["linear_velocity"].tobytes() == p["v32"].tobytes() and record["angular_velocity"].tobytes() == p["w32"].tobytes(), what
    worst = 0.0
    for i in range(3):
        for j in range(3):
            want, mag = p["R"][i][j]
            err = abs(Fraction(float(record["transform"][3 * i + j])) - want)
            slack = T.C_R * T.U * mag
            assert err <= T.U32 * (abs(want) + slack) + slack, (what, i, j)
            worst = max(worst, float(err / (T.U32 * abs(want) + slack)) if want or slack else 0.0)
    return worst


def unit_length(q):
    """| |q| - 1 | <= 4 u (the bound of test_bodies_step.py's unit-length test: 3.5 u from the division, the root and the sum of squares),
    with | n2 - 1 | ~ 2 | |q| - 1 | summed exactly"""
    return abs(sum(c * c for c in T.exact(q)) - 1) / 2 <= 4 * T.U


# ---- 1. random substeps against the twin -----------------------------------------------------------------------------------------------------

def test_random_substeps_are_the_twins_within_the_rounding_counts(harness):
    st, res, dts = random_rigid_states(320, seed=20261020)
    worst, worst_pose = {}, 0.0
    for i in range(len(st)):
        after, flag = finish(harness, st[i], res[i], dts[i])
        assert flag == 0, i
        assert hold_step(st[i], res[i], after, dts[i], worst, i), i
        assert not np.array_equal(after["orientation"], st["orientation"][i]) and not np.array_equal(after["angular_velocity"], st["angular_velocity"][i])
        assert unit_length(after["orientation"]), i                      # whatever the length of the one that went in
        rec = np.zeros(1, W.BUOYANCY_BODY)
        harness.harness_rigid_pose(st[i:i + 1].ctypes.data, rec.ctypes.data)
        worst_pose = max(worst_pose, hold_pose(rec[0], st[i], i))
    report("320 random substeps, CPU build", worst)
    print(f"pose records: worst R error / (FP32 rounding + C_R u magnitude) {worst_pose:.3f}")


def test_bodies_that_are_not_integrated_come_back_byte_for_byte(harness):
    st, res, dts = random_rigid_states(12, seed=7)
    st["mass"][0], st["mass"][1] = 0.0, -3.0                        # kinematic
    st["orientation"][2] = 0.0                                      # no length
    st["position"][3, 1], st["applied_torque"][4, 2], st["mass"][5] = np.nan, np.inf, np.inf
    st["orientation"][6] = (1e200, 0, 0, 1e200)                     # its squared length is not finite
    st["linear_drag"][7] = np.inf
    flags_in = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0]                 # 8, 9: sound and dynamic, but flagged
    for i in range(len(st)):
        after, flag = finish(harness, st[i], res[i], dts[i], flags_in[i])
        if i < 10:
            assert T.step(st[i], res[i], dts[i], G32, flags_in[i]) is None, i
            assert after.tobytes() == st[i].tobytes(), i
            assert flag == (1 if 2 <= i <= 9 else 0), i
            assert T.pose(st[i])["ok"] == (i in (0, 1, 8, 9)), i
        else:
            assert flag == 0 and hold_step(st[i], res[i], after, dts[i], {}, i)


# ---- 2. the basis by hand --------------------------------------------------------------------------------------------------------------------

def basis_bound(iinv, dt):
    """w = dt (tau Iinv): tau = 0 + Ta, tau * Iinv and dt * (..) round at most once each (R's entries are 0 and 1 here, so its products and
    the sums with zeros are exact, as is 0 + dt (..)): (exact, ((1 + u)^3 - 1) | exact |)"""
    want = Fraction(dt) * Fraction(BASIS_TORQUE) * Fraction(iinv)
    return want, ((1 + T.U) ** 3 - 1) * abs(want)


def check_basis(after, before, cases, dt):
    for b, (world, body, locked) in enumerate(cases):
        if before["mass"][b] <= 0:
            assert after[b].tobytes() == before[b].tobytes()
            continue
        w = after["angular_velocity"][b]
        sign = -1 if before["applied_torque"][b, world] < 0 else 1
        if locked:
            assert w.tobytes() == np.zeros(3).tobytes(), (b, w)          # +0.0 in every component, bit for bit
            assert after["orientation"][b].tobytes() == before["orientation"][b].tobytes()
            continue
        want, bound = basis_bound(before["inverse_inertia"][b, body], dt)
        assert abs(Fraction(float(w[world])) - sign * want) <= bound, (b, w)
        assert w[world] != 0 and all(w[k] == 0 for k in range(3) if k != world), (b, w)


def test_the_basis_by_hand_at_the_half_quaternion(harness):
    """q = (1/2, 1/2, 1/2, 1/2) carries body x to world y, y to z and z to x: a torque along world y must meet Iinv_x = a, along z Iinv_y = b,
    along x Iinv_z = c; with R transposed a torque along y would meet c.  The other two components stay exactly 0, a locked axis keeps all
    three at +0.0."""
    st, _, cases = basis_bodies()
    zero = np.zeros(1, W.BUOYANCY_RESULT)
    dt = 1.0 / 60.0
    after = st.copy()
    for b in range(len(st)):
        after[b], flag = finish(harness, st[b], zero[0], dt)
        assert flag == 0
    check_basis(after, st, cases, dt)
    assert len(set(BASIS_IINV)) == 3 and [c[:2] for c in cases[:3]] == [(1, 0), (2, 1), (0, 2)]


# ---- 3. spherical inertia --------------------------------------------------------------------------------------------------------------------

def test_spherical_inertia_turns_the_body_about_the_torque(harness):
    """Iinv = (s, s, s): R diag(s) R^T tau = s tau for a unit q whatever the orientation, so w_K = K dt s tau and v_x,K = K dt Fa / m.  The
    differences telescope: | w_K - K dt s tau | <= sum_k | w_k+1 - (w_k + dt s tau) |, each term at most the twin's bound for that substep
    (from the state the build was in) plus what the twin's own step differs from dt s tau by because the build's q is not exactly of unit
    length: with | q |^2 = 1 + e, R(q) = (1 + e) R^ - e I for the rotation R^, so R R^T - I = (2 e + 2 e^2) I - e (1 + e) (R^ + R^^T) and
    | ((R R^T - I) tau)_i | <= 2 |e| (1 + |e|) (| tau_i | + sum_j | tau_j |); e is taken exactly from the state."""
    d, sc = calm()
    K, dt, s = 64, 1.0 / 120.0, 0.0173
    tau, fa = (310.0, -95.5, 41.25), 777.0
    rng = np.random.default_rng(3)
    q0 = rng.normal(size=4)
    st, hull = make_bodies([crate(origin=(1.0, 200.0, -2.0), q=tuple(q0 / np.linalg.norm(q0)), force=(fa, 0, 0), torque=tau, kl=3.0, kq=0.5)])
    st["inverse_inertia"][0] = s
    cs = CpuSet(harness, st, hull)
    bound_w, bound_v, worst = [Fraction(0)] * 3, Fraction(0), {}
    ft, fdt, fs = [Fraction(t) for t in tau], Fraction(dt), Fraction(s)
    for k in range(K):
        before = cs.state[0].copy()
        cs.step(d, sc, 1, dt)
        assert (cs.results["force"] == 0).all() and (cs.results["torque"] == 0).all() and cs.flags[0] == 0
        hold_step(before, cs.results[0], cs.state[0], dt, worst, k)
        stepped = T.step(before, cs.results[0], dt, G32)
        e = abs(sum(c * c for c in T.exact(before["orientation"])) - 1)
        for i in range(3):
            bound_w[i] += T.C_W * T.U * stepped["w"][i][1] + fdt * fs * 2 * e * (1 + e) * (abs(ft[i]) + sum(abs(t) for t in ft))
        bound_v += T.C_V * T.U * stepped["v"][0][1]
    m = Fraction(float(st["mass"][0]))
    for i in range(3):
        err = abs(Fraction(float(cs.state["angular_velocity"][0, i])) - K * fdt * fs * ft[i])
        print(f"w[{i}] after {K} substeps: error {float(err):.3e}, bound {float(bound_w[i]):.3e}")
        assert err <= bound_w[i]
    err = abs(Fraction(float(cs.state["linear_velocity"][0, 0])) - K * fdt * Fraction(fa) / m)
    print(f"v_x after {K} substeps: error {float(err):.3e}, bound {float(bound_v):.3e}")
    assert err <= bound_v
    assert cs.state["linear_velocity"][0, 2] == 0
    report("spherical inertia, 64 substeps", worst)


# ---- 4. a torque-free spin: the orientation itself -------------------------------------------------------------------------------------------

SPIN_K, SPIN_DT = 1000, 1.0 / 120.0


def spin_closed_form(q0, w, K, dt, order="world"):
    """q_K of a torque-free spin as four floats-to-be (extended precision): q + h (w, 0) (x) q = (h w, 1) (x) q, and (h w, 1) / sqrt(1 + h^2 |w|^2)
    is the rotation about w^ by 2 atan(|w| h), so q_K = rot(w^, 2 K atan(|w| dt / 2)) (x) q0 / |q0| -- trigonometry at 60 digits (mpmath)
    where it is installed.  Without it, and as a check on it, De Moivre in exact rationals: (h w, 1)^K / (1 + h^2 |w|^2)^(K / 2) for an even
    K.  order "body": q0 (x) rot, what an integrator that takes w in body axes would give."""
    fq, fw, h = T.exact(q0), T.exact(w), Fraction(float(dt)) / 2
    n0 = T.sqrt_fraction(sum(c * c for c in fq))
    unit0 = [c / n0 for c in fq]
    assert K % 2 == 0
    den = 1
    for c in fw:
        den = max(den, (h * c).denominator)                     # powers of two: the largest is the common one
    base, p, k = [int(h * c * den) for c in fw] + [den], [0, 0, 0, 1], K
    while k:                                                    # (h w, 1)^K den^K in integers, by squaring: powers of one quaternion commute
        if k & 1:
            p = T.hamilton(p, base)
        base, k = T.hamilton(base, base), k >> 1
    scale = sum(c * c for c in [int(h * c * den) for c in fw] + [den]) ** (K // 2)
    rot = [Fraction((c << 300) // scale, 2 ** 300) for c in p]   # within 2^-300
    try:
        import mpmath
    except ImportError:
        mpmath = None
    if mpmath is not None:
        with mpmath.workdps(60):
            mw = [mpmath.mpf(c.numerator) / c.denominator for c in fw]
            mh = mpmath.mpf(h.numerator) / h.denominator
            wn = mpmath.sqrt(sum(c * c for c in mw))
            half = K * mpmath.atan(wn * mh)                      # half the angle
            trig = [c / wn * mpmath.sin(half) for c in mw] + [mpmath.cos(half)]
            for a, b in zip(trig, rot):
                assert abs(a - mpmath.mpf(b.numerator) / b.denominator) < mpmath.mpf(10) ** -50
            rot = [Fraction(int(mpmath.floor(c * 2 ** 200)), 2 ** 200) for c in trig]
    return T.hamilton(rot, unit0) if order == "world" else T.hamilton(unit0, rot)


def spin_bound(L, state, K, dt):
    """The bound on | q_K - closed form | for one spinning body: the build's substep from q_k lands within e_k = C_Q u magnitude_k (the
    twin's, per component) of rot (x) q_k / |q_k|; every later substep multiplies by a unit quaternion and renormalises, which moves no two
    quaternions of about unit length further apart (to first order: an isometry and a projection onto the sphere), so the errors add:
    | q_K - closed form |_2 <= sum_k | e_k |_2, and no component is further off than the whole.  Walked along the CPU build's trajectory
    (the twin's magnitudes depend on the state), with a zero record and no gravity's influence on q.  Returns (bound, the final state)."""
    zero = np.zeros(1, W.BUOYANCY_RESULT)[0]
    s, total = np.array(state, W.RIGID_BODY).reshape(1).copy()[0], Fraction(0)
    for _ in range(K):
        stepped = T.step(s, zero, dt, G32)
        e = T.sqrt_fraction(sum((T.C_Q * T.U * mag) ** 2 for _, mag in stepped["q"]), bits=64)
        total += Fraction(int(e * (1 + Fraction(1, 2 ** 60)) * 2 ** 160) + 1, 2 ** 160)   # rounded up (the root is from below) onto one denominator
        s, flag = finish(L, s, zero, dt)
        assert flag == 0
    return total, s


@pytest.fixture(scope="module")
def spin_case(harness):
    """the seven spinning bodies, their closed forms after SPIN_K substeps and the bounds, computed once"""
    st, hull = spin_bodies()
    want, bound, final = [], [], []
    for b in range(len(st)):
        if st["mass"][b] <= 0:
            want.append(None), bound.append(None), final.append(st[b].copy())
            continue
        want.append(spin_closed_form(st["orientation"][b], st["angular_velocity"][b], SPIN_K, SPIN_DT))
        bd, s = spin_bound(harness, st[b], SPIN_K, SPIN_DT)
        bound.append(bd), final.append(s)
    return st, hull, want, bound, final


def check_spin(after, spin_case, title):
    st, _, want, bound, _ = spin_case
    for b in range(len(st)):
        if want[b] is None:
            assert after[b].tobytes() == st[b].tobytes()
            continue
        assert after["angular_velocity"][b].tobytes() == st["angular_velocity"][b].tobytes(), b    # no torque: w does not move at all
        err = [abs(g - w) for g, w in zip(T.exact(after["orientation"][b]), want[b])]
        norm = T.sqrt_fraction(sum(e * e for e in err)) if any(err) else Fraction(0)
        print(f"{title}, body {b}: | q_K - closed form | {float(norm) / float(T.U):.1f} u (bound {float(bound[b] / T.U):.0f} u)")
        assert norm * (1 + Fraction(1, 2 ** 100)) <= bound[b], b


def test_a_torque_free_spin_lands_on_the_rotation_it_must_be(harness, spin_case):
    st, hull, want, bound, final = spin_case
    d, sc = calm()
    cs = CpuSet(harness, st, hull)
    done = 0
    while done < SPIN_K:
        k = min(250, SPIN_K - done)
        cs.step(d, sc, k, SPIN_DT)
        done += k
    assert (cs.flags == 0).all() and (cs.results["wetted_points"] == 0).all()
    check_spin(cs.state, spin_case, "CPU build")
    for b in range(len(st)):       # the substep loop around the hull and the bare integrator walked for the bound are the same build
        assert cs.state["orientation"][b].tobytes() == final[b]["orientation"].tobytes()
    # the case tells the two product orders apart, on the references alone: w in body axes would land far from the closed form
    body = spin_closed_form(st["orientation"][0], st["angular_velocity"][0], SPIN_K, SPIN_DT, order="body")
    apart = max(abs(a - b) for a, b in zip(body, want[0]))
    print(f"q0 (x) rot is {float(apart):.3f} from rot (x) q0")
    assert apart > Fraction(1, 1000)
    assert st["orientation"][0].tobytes() == quaternion(*SPIN_Q0).tobytes() and tuple(st["angular_velocity"][0]) == SPIN_W


# ---- 5. a tilted box rights itself -----------------------------------------------------------------------------------------------------------

def tilt_of(state):
    x, _, z, _ = state["orientation"]
    return float(np.arccos(min(1.0, 1.0 - 2.0 * (x * x + z * z))))


@pytest.mark.parametrize("axis,angle", [((1, 0, 0), 0.25), ((1, 0, 0), -0.25), ((0, 0, 1), 0.25), ((0, 0, 1), -0.25)])
def test_a_tilted_box_rights_itself(harness, axis, angle):
    """Conditions, not measurements: the buoyant torque of a wide box opposes its tilt and the drag only removes energy, so the first
    substep turns it back about the tilt axis alone (R of a rotation about x or z has exact zeros, and the other two torque components sum
    symmetric hull points to exactly 0), the tilt acos(R_11) never exceeds the initial one and it dies away."""
    d, sc = calm()
    st, hull = tilted_box(axis, angle)
    cs = CpuSet(harness, st, hull)
    k = axis.index(1)
    tilt0 = tilt_of(st[0])
    assert abs(tilt0 - 0.25) < 1e-12
    largest = 0.0
    for step in range(1200):
        cs.step(d, sc, 1, 1.0 / 120.0, {"warm_start": True})
        if step == 0:
            w = cs.state["angular_velocity"][0]
            assert cs.results["wetted_points"][0] > 0 and cs.results["torque"][0, k] * angle < 0
            assert w[k] * angle < 0 and all(w[j] == 0 for j in range(3) if j != k), w
        largest = max(largest, tilt_of(cs.state[0]))
        assert largest <= tilt0, step
    final = tilt_of(cs.state[0])
    print(f"tilt {angle:+.2f} about {axis}: largest tilt on the way {largest:.6f} (initial {tilt0:.6f}), final {final:.3e}")
    assert final < 1e-6
    assert cs.flags[0] == 0 and (cs.results["invalid_points"] == 0).all()


# ---- 6. saturation of the pose record --------------------------------------------------------------------------------------------------------

def all_finite(*arrays):
    for arr in arrays:
        for f in arr.dtype.names:
            if arr[f].dtype.kind == "f":
                assert np.isfinite(arr[f]).all(), f


def check_saturated(state, records, before):
    """the pose records of saturated_bodies' states: +-FLT_MAX where the FP64 state exceeds it, the FP32 narrowing elsewhere"""
    for b in range(len(state)):
        hold_pose(records[b], state[b], b)
    o = records["transform"][:, 9:]
    assert o[0, 0] == np.float32(FLT_MAX) and o[0, 2] == np.float32(-FLT_MAX) and o[1, 0] == np.float32(FLT_MAX) and o[2, 1] == np.float32(-FLT_MAX)
    assert records["linear_velocity"][1, 0] == np.float32(FLT_MAX) and records["angular_velocity"][2, 1] == np.float32(-FLT_MAX)
    assert state["position"][1, 0] > before["position"][1, 0] > FLT_MAX          # FP64 goes on: the fast body moves,
    assert (state["linear_velocity"][:, 1] != before["linear_velocity"][:, 1]).all()   # gravity, buoyancy or drag reach every body
    assert not np.array_equal(state["orientation"][2], before["orientation"][2])       # and the spinning one turns
    assert unit_length(state["orientation"][2])


def test_pose_records_saturate_and_the_state_goes_on_in_fp64(harness):
    d, sc = calm()
    st, hull = saturated_bodies()
    cs = CpuSet(harness, st, hull)
    worst = {}
    for k in range(3):
        before = cs.state.copy()
        cs.step(d, sc, 1, 1.0 / 120.0)
        all_finite(cs.records, cs.results, cs.pts)
        assert (cs.flags == 0).all()
        for b in range(len(st)):
            assert hold_step(before[b], cs.results[b], cs.state[b], 1.0 / 120.0, worst, (k, b))
    check_saturated(cs.state, cs.records, st)
    report("saturated states, CPU build", worst)


# ---- 7-9. on the GPU -------------------------------------------------------------------------------------------------------------------------

def context(kernels, ticks=3):
    """256^2, the two cascades init_gpu takes at the least, `ticks` ticks in: (generator, map scales)"""
    from godotoceanwaves_amd import WaveCascadeParameters
    gen = W()
    gen.map_size = 256
    gen.bodies_kernels = kernels
    gen.init_gpu(2)
    params = [WaveCascadeParameters(**cascade_preset(ci)) for ci in (0, 1)]
    if ticks:
        gen.run(UPDATE_DELTA, params, ticks)
    return gen, scales_of(params)


def device_single_steps(gen, s, sc, calls, dt, opts, title):
    """`calls` calls of one substep, each held to the twin's step of the state read before it from the record read back after it.  Returns
    the result records of every call"""
    worst, records = {}, []
    before = gen.bodies_state(s)
    for k in range(calls):
        gen.bodies_step(s, sc, 1, dt, opts)
        after, res = gen.bodies_state(s), gen.bodies_results(s)
        for b in range(len(before)):
            hold_step(before[b], res[b], after[b], dt, worst, (title, k, b))
        ptr, _, _ = gen.bodies_device_ptrs(s)
        poses = device_read(ptr, s.num_bodies, W.BUOYANCY_BODY)
        for b in range(len(after)):
            hold_pose(poses[b], after[b], (title, k, b))
        records.append(res)
        before = after
    assert gen.bodies_stats(s)["faulted_bodies"] == 0
    report(title, worst)
    return records, before


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["fused", "split"])
def test_gpu_single_substeps_in_the_air_are_the_twins(kernels):
    gen, sc = context(kernels)
    st, hull = airborne_bodies()
    s = gen.bodies_create(st, hull)
    records, last = device_single_steps(gen, s, sc, 16, 1.0 / 120.0, None, f"GPU {kernels}, 16 substeps in the air")
    for res in records:
        assert (res["force"] == 0).all() and (res["torque"] == 0).all() and (res["submerged_volume"] == 0).all()
        assert (res["wetted_points"] == 0).all() and (res["invalid_points"] == 0).all()
    assert last[6].tobytes() == st[6].tobytes()                      # the kinematic body, throughout (hold_step asked after every call)
    assert last["angular_velocity"][2, 0] != st["angular_velocity"][2, 0]      # the body with a locked axis still turns about the others
    gen.bodies_destroy(s)


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["fused", "split"])
def test_gpu_single_substeps_on_the_water_are_the_twins(kernels):
    gen, sc = context(kernels)
    gen.update_velocity()
    st, hull = seven_bodies(seed=7)
    for opts in ({"warm_start": True}, {"warm_start": True, "water_velocity": True}):
        s = gen.bodies_create(st, hull)
        records, last = device_single_steps(gen, s, sc, 8, 1.0 / 120.0, opts, f"GPU {kernels}, 8 substeps on the water, {sorted(opts)}")
        wet = [(res["wetted_points"] > 0) & (np.abs(res["torque"]).max(axis=1) > 0) for res in records]
        assert np.any(wet), "no body touched the water: the case tests nothing"
        assert np.all([res["invalid_points"] == 0 for res in records])
        assert last[6].tobytes() == st[6].tobytes()
        gen.bodies_destroy(s)


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["fused", "split"])
def test_gpu_closed_forms(harness, spin_case, kernels):
    """the half-quaternion basis, the torque-free spin (1000 substeps, in calls of at most OW_BODIES_MAX_SUBSTEPS) and the saturated poses
    through ow_bodies_create, ow_bodies_step and ow_bodies_get_state, to the CPU tests' bounds"""
    gen, sc = context(kernels)
    st, hull, cases = basis_bodies()
    s = gen.bodies_create(st, hull)
    gen.bodies_step(s, sc, 1, 1.0 / 60.0)
    check_basis(gen.bodies_state(s), st, cases, 1.0 / 60.0)
    assert (gen.bodies_results(s)["wetted_points"] == 0).all()
    gen.bodies_destroy(s)

    st, hull = spin_case[0], spin_case[1]
    s = gen.bodies_create(st, hull)
    done = 0
    while done < SPIN_K:
        k = min(MAX_SUBSTEPS, SPIN_K - done)
        gen.bodies_step(s, sc, k, SPIN_DT)
        done += k
    after = gen.bodies_state(s)
    stats = gen.bodies_stats(s)
    assert stats["substeps"] == SPIN_K and stats["faulted_bodies"] == 0 and (stats["split_calls"] == 0) == (kernels == "fused")
    assert (gen.bodies_results(s)["wetted_points"] == 0).all()
    check_spin(after, spin_case, f"GPU {kernels}")
    gen.bodies_destroy(s)

    st, hull = saturated_bodies()
    s = gen.bodies_create(st, hull)
    worst = {}
    before = gen.bodies_state(s)
    for k in range(3):
        gen.bodies_step(s, sc, 1, 1.0 / 120.0)
        after, res = gen.bodies_state(s), gen.bodies_results(s)
        ptr, _, pts = gen.bodies_device_ptrs(s)
        poses = device_read(ptr, s.num_bodies, W.BUOYANCY_BODY)
        all_finite(poses, res, device_read(pts, s.num_points, W.BUOYANCY_POINT))
        for b in range(len(st)):
            assert hold_step(before[b], res[b], after[b], 1.0 / 120.0, worst, (k, b))
        before = after
    assert gen.bodies_stats(s)["faulted_bodies"] == 0
    check_saturated(after, poses, st)
    report(f"GPU {kernels}, saturated states", worst)
    gen.bodies_destroy(s)
