"""Floating bodies stepped on the device (include/ocean_waves.h ow_bodies_create, ow_bodies_step, ...; godotoceanwaves_amd/csrc/ow_rigid.h).

CPU: the ABI (header, exports, ctypes, NumPy, C and C# layouts), the argument checks without a device, the example's C99 build; ow_rigid.h
over ow_buoyancy.h compiled as plain C++ (tests/bodies/bodies_harness.cpp, g++ -ffp-contract=off, looping substeps as the fused kernel does)
held to the closed form of semi-implicit Euler in free fall, to Archimedes on a calm sea, to the existing CPU build of ow_buoyancy.h at
every pose it visits on demo-scene maps, and to itself (K substeps in one call = K calls).  GPU: states, pose records, results and point
records are the CPU build's bit for bit (cold, warm, with the falloff, on moving water); the fused kernel, the split form and the default
rule agree; the step equals a host loop around ow_buoyancy_async; it is ordered like ow_buoyancy_async, on a caller's stream too; faulted
layers are refused; examples/floating_bodies_host.c floats its crates without a host synchronisation."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from godotoceanwaves_amd import _lib, build
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import checks as S
from checks import check_declared_and_bound, exported_symbols, HEADER
from cpu_builds import build_example, cpu_buoyancy, CpuSet, CSRC, layout_probe, ROOT
from cpu_builds import bodies_harness as harness, buoyancy_harness  # noqa: F401 (fixtures)
from scenes import calm, crate, demo_bodies, device_read, generated_maps, gpu_arrays, gpu_maps, make_bodies, quaternion, RHO, scales_of

NEW_FUNCTIONS = ("ow_sync_stats", "ow_bodies_create", "ow_bodies_destroy", "ow_bodies_step", "ow_bodies_get_state", "ow_bodies_set_state", "ow_bodies_get_results",
                 "ow_bodies_get_device_ptrs", "ow_bodies_stats")
STRUCTS = {"OwRigidBody": "ow_rigid_body", "OwBodiesOptions": "ow_bodies_options"}
G32 = float(np.float32(9.81))      # the gravity the integrator uses: the FP32 default of ow_buoyancy_options, widened
U = 2.0 ** -53                     # FP64 unit roundoff


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_body_set_and_the_library_exports_it():
    build.build_library()
    lib = _lib.load()
    text = check_declared_and_bound(lib, NEW_FUNCTIONS)
    for struct in STRUCTS.values():
        assert re.search(r"typedef struct %s \{" % struct, text), struct
    assert re.search(r"typedef struct ow_bodies ow_bodies;", text)
    assert set(NEW_FUNCTIONS) <= exported_symbols()
    assert lib.ow_abi_version() == 4   # symbols were added, nothing changed
    assert "NO GYROSCOPIC TERM" in open(os.path.join(CSRC, "ow_rigid.h")).read()   # the header says what the integrator leaves out
    assert "There is no group form (ow_group_*)" in HEADER


def test_body_structs_agree_in_c_ctypes_numpy_and_the_harness(tmp_path, harness):
    fields = []
    for c in STRUCTS.values():
        ct = getattr(_lib, c)
        fields += [(c, None)] + [(c, f) for f, _ in ct._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ocean_waves.h"\nint main(void){\n'
    for c, f in fields:
        src += '    printf("%%zu\\n", %s);\n' % (f"sizeof({c})" if f is None else f"offsetof({c}, {f})")
    src += '    printf("%u %u %d\\n", OW_FLAG_BODIES_FUSED, OW_FLAG_BODIES_SPLIT, OW_BODIES_MAX_SUBSTEPS);\n    return 0;\n}\n'
    got = layout_probe(tmp_path, "bodies_layout", src, std=("-std=c99", "-pedantic", "-Wall", "-Werror"))
    want = []
    for c, f in fields:
        ct = getattr(_lib, c)
        want.append(C.sizeof(ct) if f is None else getattr(ct, f).offset)
    want += [_lib.OW_FLAG_BODIES_FUSED, _lib.OW_FLAG_BODIES_SPLIT, _lib.OW_BODIES_MAX_SUBSTEPS]
    assert got == want
    for c, dt in {"ow_rigid_body": W.RIGID_BODY, "ow_bodies_options": W.BODIES_OPTIONS}.items():
        ct = getattr(_lib, c)
        assert dt.itemsize == C.sizeof(ct) and dt.names == tuple(f for f, _ in ct._fields_), c
        assert all(dt.fields[f][1] == getattr(ct, f).offset for f in dt.names), c
    assert [C.sizeof(getattr(_lib, c)) for c in STRUCTS.values()] == [208, 80]
    sizes = (C.c_int * 7)()
    harness.harness_bodies_sizes(sizes)
    R = _lib.ow_rigid_body
    assert list(sizes) == [208, R.orientation.offset, R.mass.offset, R.inverse_inertia.offset, R.applied_torque.offset, R.linear_drag.offset,
                           R.point_offset.offset]


def test_the_csharp_binding_shows_the_body_structs_and_functions():
    c_sizes = dict(S.C_SIZES, ow_buoyancy_options=64)
    cs_sizes = dict(S.CS_SIZES, OwBuoyancyOptions=64)

    def fields(body, sizes, strip):
        out = []
        for decl in body.split(";"):
            decl = " ".join(strip(decl).split())
            if not decl:
                continue
            decl = decl[len("fixed "):] if decl.startswith("fixed ") else decl
            typ, names = decl.split(" ", 1)
            for n in names.split(","):
                m = re.match(r"\s*([A-Za-z_]\w*)(\[(\d+)\])?\s*$", n)
                out.append((m.group(1), sizes[typ] * int(m.group(3) or 1)))
        return out

    for cs, c in STRUCTS.items():
        cbody = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (c, c), S.strip_comments(S.HEADER), flags=re.S).group(1)
        csbody = re.search(r"struct %s \{(.*?)\n\}" % cs, S.strip_comments(S.SHIM), flags=re.S).group(1)
        want = fields(cbody, c_sizes, lambda d: d)
        got = fields(csbody, cs_sizes, lambda d: d.replace("public", ""))
        assert got == want, (cs, got, want)
        assert sum(s for _, s in want) == C.sizeof(getattr(_lib, c)), c
    cfun = S.c_functions()
    for name in NEW_FUNCTIONS:
        m = re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:int|void) %s\((.*?)\);" % name, S.SHIM)
        assert m, name
        assert m.group(1).count(",") + 1 == cfun[name][1], name
        assert "`%s`" % name in S.DOC.split("## 7. Index")[1], name


# ---- 2. argument checks without a device ---------------------------------------------------------------------------------------------

def test_argument_errors_without_a_device():
    """the host checks run before the context is looked at: each bad argument is named, and nothing is written"""
    lib = _lib.load()
    st, hull = make_bodies([crate(origin=(0, 0, 0)), crate(origin=(5, 0, 0), divisions=(2, 1, 2))])

    def create(s, h):
        out = C.c_void_p(0x5A5A)
        code = lib.ow_bodies_create(None, s.ctypes.data, len(s), h.ctypes.data, len(h), C.byref(out))
        assert not out.value   # no handle comes back from a refused call
        return code, lib.ow_last_error()

    def bad(s, h, word):
        code, msg = create(s, h)
        assert code == _lib.OW_ERR_INVALID and word in msg, msg

    h = hull.copy()
    h["volume"][3] = -1.0
    bad(st, h, b"volume")
    h = hull.copy()
    h["body"][2] = 1
    bad(st, h, b"names body")
    h = hull.copy()
    h["local"][5, 1] = np.inf
    bad(st, h, b"finite")
    s = st.copy()
    s["point_count"][1] += 1
    bad(s, hull, b"outside")
    for field, word in (("position", b"finite"), ("linear_velocity", b"finite"), ("angular_velocity", b"finite"), ("applied_force", b"finite"),
                        ("applied_torque", b"finite"), ("inverse_inertia", b"finite")):
        s = st.copy()
        s[field][1, 2] = np.nan
        bad(s, hull, word)
    s = st.copy()
    s["mass"][0] = np.inf
    bad(s, hull, b"mass")
    s = st.copy()
    s["inverse_inertia"][0, 0] = -1.0
    bad(s, hull, b"inverse_inertia")
    s = st.copy()
    s["orientation"][1] = (0, 0, 0, 0)
    bad(s, hull, b"unit quaternion")
    s = st.copy()
    s["orientation"][1] = (0, 0, 0, 1.001)
    bad(s, hull, b"unit quaternion")
    s = st.copy()
    s["orientation"][0, 0] = np.nan
    bad(s, hull, b"quaternion")
    s = st.copy()
    s["reserved"][0, 1] = 7
    bad(s, hull, b"reserved")
    assert lib.ow_bodies_create(None, st.ctypes.data, 0, hull.ctypes.data, len(hull), C.byref(C.c_void_p())) == _lib.OW_ERR_INVALID
    code, msg = create(st, hull)    # everything checkable is fine: only the missing context is left
    assert code == _lib.OW_ERR_INVALID and b"null context" in msg, msg

    sc = np.ones((1, 4), np.float32)

    def step(substeps, dt, opts=None):
        code = lib.ow_bodies_step(None, None, sc.ctypes.data, 1, C.byref(opts) if opts is not None else None, substeps, dt)
        return code, lib.ow_last_error()

    for k in (0, -1, _lib.OW_BODIES_MAX_SUBSTEPS + 1):
        code, msg = step(k, 1 / 60)
        assert code == _lib.OW_ERR_INVALID and b"substeps" in msg
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        code, msg = step(4, dt)
        assert code == _lib.OW_ERR_INVALID and b"dt" in msg
    o = _lib.ow_bodies_options()
    o.reserved[2] = 1
    code, msg = step(4, 1 / 60, o)
    assert code == _lib.OW_ERR_INVALID and b"reserved" in msg
    o = W.bodies_options({"density": float("nan")})
    code, msg = step(4, 1 / 60, o)
    assert code == _lib.OW_ERR_INVALID and b"finite" in msg
    o = _lib.ow_bodies_options()
    o.buoyancy.flags = 0x10
    code, msg = step(4, 1 / 60, o)
    assert code == _lib.OW_ERR_INVALID and b"flags" in msg
    code, msg = step(4, 1 / 60)
    assert code == _lib.OW_ERR_INVALID and b"null" in msg
    rec = np.frombuffer(np.full(208, 0xA5, np.uint8).tobytes(), W.RIGID_BODY).copy()
    before = rec.tobytes()
    assert lib.ow_bodies_get_state(None, None, 0, 1, rec.ctypes.data) == _lib.OW_ERR_INVALID and rec.tobytes() == before
    assert lib.ow_bodies_set_state(None, None, 0, 1, rec.ctypes.data) == _lib.OW_ERR_INVALID
    assert lib.ow_bodies_get_results(None, None, 0, 1, rec.ctypes.data) == _lib.OW_ERR_INVALID and rec.tobytes() == before
    assert lib.ow_bodies_get_device_ptrs(None, None, None, None, None) == _lib.OW_ERR_INVALID
    assert lib.ow_bodies_stats(None, None, None, None, None, None) == _lib.OW_ERR_INVALID
    lib.ow_bodies_destroy(None, None)   # allowed
    m, iinv = W.box_mass_properties((2.0, 1.0, 4.0), 500.0)
    assert m == 4000.0 and np.allclose(iinv, (12 / (m * 17), 12 / (m * 20), 12 / (m * 5)))


def test_example_builds_as_pedantic_c99(tmp_path):
    build.build_library()
    exe = build_example(tmp_path, "floating_bodies_host")
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "10"], capture_output=True, text=True)
        assert r.returncode == 1 and "no CPU fallback" in r.stderr


# ---- 3. free fall ------------------------------------------------------------------------------------------------------------------------

def test_free_fall_follows_the_closed_form_of_semi_implicit_euler(harness):
    """A body that never touches the water (1000 m up, map_scales.z = 0): every force record is zero, so per substep v += fl(dt * a) with
    a = 0 / m + (-g) = -g exactly, and y += fl(dt * v).  Against the exact v_K = -g K dt and y_K = y_0 - g dt^2 K (K + 1) / 2 (rationals):
      v: one rounding of the product dt * g (relative u) carried K times, and K additions, each rounding by at most u |v_K| (the partial
         sums grow monotonically): |error| <= (K + 1) u |v_K|; one more u |v_K| covers the second-order terms -> (K + 2) u g K dt.
      y: term j is dt * v_j with v_j off by (j + 2) u g j dt and the product rounded (u g j dt^2), and each of the K additions rounds by at
         most u y_0 (y stays in [0, y_0]): |error| <= u (g dt^2 sum_j (j (j + 2) + j) + K y_0).
    The applied force F_a along x adds one rounding, of F_a / m: |v_x error| <= (K + 3) u |v_x|.  w sees no torque and must not move at all."""
    d, sc = calm()
    K, dt, y0 = 1000, 1.0 / 240.0, 1000.0
    fa, w0 = 321.0, (0.3, -0.2, 0.5)
    st, hull = make_bodies([crate(origin=(3.0, y0, -2.0), w=w0, force=(fa, 0, 0), kl=0.5, kq=0.2), crate(origin=(0.0, y0, 0.0))])
    cs = CpuSet(harness, st, hull)
    cs.step(d, sc, K, dt)
    assert (cs.results["force"] == 0).all() and (cs.results["wetted_points"] == 0).all() and (cs.flags == 0).all()
    g, fdt = Fraction(G32), Fraction(dt)
    v_exact = -g * K * fdt
    y_exact = Fraction(y0) - g * fdt * fdt * K * (K + 1) / 2
    bound_v = (K + 2) * U * float(-v_exact)
    bound_y = U * (G32 * dt * dt * sum(j * (j + 2) + j for j in range(1, K + 1)) + K * y0)
    for b in range(2):
        ev = abs(Fraction(float(cs.state["linear_velocity"][b, 1])) - v_exact)
        ey = abs(Fraction(float(cs.state["position"][b, 1])) - y_exact)
        print(f"body {b}: |v error| {float(ev):.3e} (bound {bound_v:.3e}), |y error| {float(ey):.3e} (bound {bound_y:.3e})")
        assert ev <= bound_v and ey <= bound_y
    m = float(st["mass"][0])
    vx_exact = Fraction(fa) / Fraction(m) * K * fdt
    evx = abs(Fraction(float(cs.state["linear_velocity"][0, 0])) - vx_exact)
    print(f"|v_x error| {float(evx):.3e} (bound {(K + 3) * U * float(vx_exact):.3e})")
    assert evx <= (K + 3) * U * float(vx_exact)
    assert cs.state["linear_velocity"][0, 2] == 0 and cs.state["linear_velocity"][1, 0] == 0
    assert cs.state["angular_velocity"][0].tobytes() == np.array(w0, np.float64).tobytes()
    assert (cs.state["angular_velocity"][1] == 0).all() and cs.state["orientation"][1].tobytes() == np.array((0, 0, 0, 1), np.float64).tobytes()


def test_the_quaternion_stays_of_unit_length(harness):
    """10^4 substeps of a spinning body in free fall.  q is renormalised every substep, so nothing accumulates: each component is one division
    (relative u) by len = sqrt(n2), n2 a sum of four squares (products u each, two levels of additions 2 u: 3 u on n2, 1.5 u on its root,
    plus the root's own u).  | |q| - 1 | <= u + 2.5 u = 3.5 u < 2 ulp(1) = 4 u; n2 is summed exactly (rationals), and | n2 - 1 | ~ 2 | |q| - 1 |."""
    d, sc = calm()
    st, hull = make_bodies([crate(origin=(0, 1e6, 0), divisions=(1, 1, 1), q=quaternion((1, 2, 3), 0.7), w=(1.1, -2.3, 0.7))])
    cs = CpuSet(harness, st, hull)
    worst = 0.0
    for _ in range(200):
        cs.step(d, sc, 50, 1.0 / 120.0)
        n2 = sum(Fraction(float(x)) ** 2 for x in cs.state["orientation"][0])
        worst = max(worst, abs(float(n2 - 1)) / 2)
    print(f"largest | |q| - 1 | over 10^4 substeps: {worst / U:.2f} u")
    assert worst <= 4 * U
    assert cs.flags[0] == 0 and not np.array_equal(cs.state["orientation"][0], st["orientation"][0])


# ---- 4. a calm sea -----------------------------------------------------------------------------------------------------------------------

def test_a_box_of_half_the_waters_density_settles_at_the_archimedes_draft(harness):
    """the bound tests/test_buoyancy.py holds `buoyancy_host calm` to: within 2 % of the Archimedes draft (half the box's height).  Once
    settled, kinetic plus potential energy does not grow: E = m v^2 / 2 + sum I w^2 / 2 + m g y + rho g A draft^2 / 2 (the hull's layers
    submerge linearly and contiguously, so the buoyant force is rho g A clamp(draft, 0, H) exactly in the model).  The forces are FP32, so
    the potential the integrator sees differs from this FP64 one by an FP32 ulp of the energy scale: the slack is 2^-23 m g H."""
    d, sc = calm()
    size = (2.0, 1.0, 2.0)
    st, hull = make_bodies([crate(size=size, origin=(5.0, 0.3, -3.0), kl=3.0, kq=0.5)])
    cs = CpuSet(harness, st, hull)
    m, A, H = float(st["mass"][0]), size[0] * size[2], size[1]
    rho_g = float(np.float32(np.float32(RHO) * np.float32(9.81)))
    energy = []
    for k in range(600):
        cs.step(d, sc, 1, 1.0 / 60.0, {"warm_start": True})
        s = cs.state[0]
        draft = min(max(-(s["position"][1] - H / 2), 0.0), H)
        inertia = 1.0 / s["inverse_inertia"]
        energy.append(0.5 * m * (s["linear_velocity"] ** 2).sum() + 0.5 * (inertia * s["angular_velocity"] ** 2).sum() + m * G32 * s["position"][1]
                      + rho_g * A * draft * draft / 2)
    draft = -(cs.state["position"][0, 1] - H / 2)
    print(f"draft {draft:.6f} against {0.5 * H}; E settles from {energy[0]:.3f} to {energy[-1]:.6f}")
    assert abs(draft - 0.5 * H) <= 0.02 * 0.5 * H
    settled = np.array(energy[300:])
    assert settled.max() <= settled[0] + 2.0 ** -23 * m * G32 * H
    assert energy[-1] < energy[0]
    assert cs.flags[0] == 0 and np.abs(cs.state["angular_velocity"][0]).max() < 1e-6


# ---- 5. demo-scene maps --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def demo_maps():
    d, _, sc = generated_maps(256, [0, 1, 2])
    return d, sc


@pytest.mark.parametrize("opts", [{}, {"warm_start": True}, {"falloff_center": (30.0, -60.0), "water_level": 0.2, "warm_start": True}])
def test_every_substep_is_the_existing_cpu_buoyancy_at_the_harness_pose(harness, buoyancy_harness, demo_maps, opts):
    d, sc = demo_maps
    st, hull = demo_bodies()
    cs = CpuSet(harness, st, hull)
    pts = np.zeros(len(hull), W.BUOYANCY_POINT)
    for k in range(12):
        tr, tb = cs.step(d, sc, 1, 1.0 / 120.0, opts, trace=True)
        want, pts = cpu_buoyancy(buoyancy_harness, d, sc, tb[0], hull, opts, points=pts if opts.get("warm_start") else None)
        assert tr[0].tobytes() == want.tobytes(), k
        assert cs.pts.tobytes() == pts.tobytes(), k
        assert cs.results.tobytes() == want.tobytes()
    assert (cs.results["wetted_points"] > 0).any() and (cs.results["invalid_points"] == 0).all() and (cs.flags == 0).all()
    moved = np.abs(cs.state["position"] - st["position"]).max(axis=1)
    assert (moved > 1e-3).all()
    # the pose record is the state narrowed: the origin to FP32, the basis from the quaternion
    assert np.array_equal(cs.records["transform"][:, 9:], cs.state["position"].astype(np.float32))
    for b in range(len(st)):
        x, y, z, w = cs.state["orientation"][b]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(cs.records["transform"][b, :9].reshape(3, 3), R, atol=1e-6)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)


def test_k_substeps_in_one_call_equal_k_calls_of_one(harness, demo_maps):
    d, sc = demo_maps
    st, hull = demo_bodies(seed=3)
    for opts in ({}, {"warm_start": True}):
        one, many = CpuSet(harness, st, hull), CpuSet(harness, st, hull)
        one.step(d, sc, 16, 1.0 / 240.0, opts)
        for _ in range(16):
            many.step(d, sc, 1, 1.0 / 240.0, opts)
        assert one.arrays() == many.arrays(), opts


# ---- 6. bad input ------------------------------------------------------------------------------------------------------------------------

def test_bad_input_puts_nothing_non_finite_into_any_record(harness, demo_maps):
    d, sc = demo_maps
    fields = ("position", "orientation", "linear_velocity", "angular_velocity", "mass", "inverse_inertia", "applied_force", "applied_torque",
              "linear_drag", "quadratic_drag")
    items = [crate(origin=(4.0 * i, 0.1, 0.0), divisions=(2, 2, 2)) for i in range(len(fields) * 2 + 5)]
    st, hull = make_bodies(items)
    bad = 0
    for bad_value in (np.nan, np.inf):
        for f in fields:
            if st[f].ndim == 1:
                st[f][bad] = bad_value
            else:
                st[f][bad, -1] = bad_value
            bad += 1
    zero_q, kinematic, negative_mass, empty, overflow = range(bad, bad + 5)
    st["orientation"][zero_q] = 0.0
    st["mass"][kinematic] = 0.0
    st["mass"][negative_mass] = -3.0
    st["position"][[kinematic, negative_mass], 1] = -5.0   # well under the demo scene's troughs
    st["point_count"][empty] = 0                    # its hull points are left to no body: the harness, like the device, counts and skips them
    st["linear_velocity"][overflow] = (0, 1.7e308, 0)   # finite now, not after the first o += dt * v
    before = st.copy()
    cs = CpuSet(harness, st, hull)
    cs.step(d, sc, 8, 10.0)
    for arr in (cs.records, cs.results, cs.pts):
        for f in arr.dtype.names:
            if arr[f].dtype.kind == "f":
                assert np.isfinite(arr[f]).all(), f
    assert list(cs.flags[:bad]) == [1] * bad and cs.flags[zero_q] == 1 and cs.flags[overflow] == 1
    assert cs.flags[kinematic] == 0 and cs.flags[negative_mass] == 0 and cs.flags[empty] == 0
    assert cs.flags.sum() == bad + 2
    # faulted on its input: the null record, nothing evaluated, the state as given
    assert (cs.records["point_count"][:bad] == 0).all() and (cs.results["force"][:bad] == 0).all()
    assert cs.state[:bad + 1].tobytes() == before[:bad + 1].tobytes()
    faulted_points = np.concatenate([np.arange(s["point_offset"], s["point_offset"] + s["point_count"]) for s in before[:bad + 1]])
    assert (cs.pts["body"][faulted_points] == -1).all()
    # kinematic: forces, no motion
    for b in (kinematic, negative_mass):
        assert cs.state[b].tobytes() == before[b].tobytes() and cs.results["wetted_points"][b] > 0 and cs.results["force"][b, 1] > 0
    # no hull: falls freely
    assert cs.results["wetted_points"][empty] == 0 and cs.state["linear_velocity"][empty, 1] < 0 and np.isfinite(cs.state["position"][empty]).all()
    # overflowed in its first substep: frozen at the state it had, which is finite
    assert cs.state[overflow].tobytes() == before[overflow].tobytes()
    for f in fields[:4]:
        assert np.isfinite(cs.state[f][bad + 1:]).all(), f


# ---- 7-13. on the GPU ----------------------------------------------------------------------------------------------------------------------

def parity_scene():
    """bodies of 1, 63, 64, 65, 200 and 1000 hull points, tilted and moving, a kinematic one among them"""
    st, hull = demo_bodies(counts=(1, 63, 64, 65, 200, 1000, 30), seed=7, spread=120.0)
    st["mass"][6] = 0.0
    return st, hull


def gen_with(n, ids, kernels=None, stream=None, ticks=3):
    from godotoceanwaves_amd import WaveCascadeParameters
    from godotoceanwaves_amd.presets import cascade_preset
    gen = W()
    gen.map_size = n
    gen.bodies_kernels = kernels
    if stream is not None:
        gen.stream = stream
    gen.init_gpu(max(2, len(ids)))
    params = [WaveCascadeParameters(**cascade_preset(ci)) for ci in ids]
    if ticks:
        gen.run(UPDATE_DELTA, params, ticks)
    return gen, params


OPTION_CASES = [{}, {"warm_start": True}, {"falloff_center": (12.5, -40.0), "water_level": 0.3, "warm_start": True},
                {"water_velocity": True, "warm_start": True}]


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["fused", "split"])
def test_gpu_states_and_records_are_the_cpu_builds_bit_for_bit(harness, kernels):
    n, ids = 512, [0, 1, 2]
    gen, params = gen_with(n, ids, kernels)
    sc = scales_of(params)
    d, _ = gpu_maps(gen, len(ids))
    gen.update_velocity()
    vel = np.stack([gen.velocity_map(i) for i in range(len(ids))])
    st, hull = parity_scene()
    dt = 1.0 / 240.0
    for opts in OPTION_CASES:
        v = vel if opts.get("water_velocity") else None
        for substeps in (1, 4, 32):
            s = gen.bodies_create(st, hull)
            cs = CpuSet(harness, st, hull)
            assert gpu_arrays(gen, s) == cs.arrays(), "as created"
            gen.bodies_step(s, sc, substeps, dt, opts)
            cs.step(d, sc, substeps, dt, opts, vel=v)
            got, want = gpu_arrays(gen, s), cs.arrays()
            for name in want:
                assert got[name] == want[name], (opts, substeps, name)
            # a second call continues from the first one's records (the warm start's state among them)
            gen.bodies_step(s, sc, 4, dt, opts)
            cs.step(d, sc, 4, dt, opts, vel=v)
            assert gpu_arrays(gen, s) == cs.arrays(), (opts, substeps, "second call")
            stats = gen.bodies_stats(s)
            assert stats["substeps"] == substeps + 4 and stats["faulted_bodies"] == 0
            assert (stats["fused_launches"], stats["split_calls"]) == ((2, 0) if kernels == "fused" else (0, 2))
            gen.bodies_destroy(s)
    moved = np.frombuffer(want["state"], W.RIGID_BODY)
    assert np.isfinite(moved["position"]).all() and moved[6].tobytes() == st[6].tobytes()   # the kinematic body stayed


@pytest.mark.gpu
def test_fused_split_and_the_default_rule_agree_and_set_state_teleports(harness):
    n, ids = 256, [0, 1, 2, 3]
    st, hull = parity_scene()
    outs, teleported = {}, {}
    for kernels in ("fused", "split", None):
        gen, params = gen_with(n, ids, kernels)
        sc = scales_of(params)
        s = gen.bodies_create(st, hull)
        gen.bodies_step(s, sc, 8, 1.0 / 120.0, {"warm_start": True})
        gen.bodies_step(s, sc, 3, 1.0 / 60.0, {"warm_start": True, "water_velocity": True})
        outs[kernels] = gpu_arrays(gen, s)
        # teleport two bodies: their warm start is reset, the others keep theirs
        new = st[[1, 4]].copy()
        new["position"][:, 0] += 50.0
        gen.bodies_set_state(s, new[:1], first=1)
        gen.bodies_set_state(s, new[1:], first=4)
        got = gpu_arrays(gen, s)
        pts = np.frombuffer(got["points"], W.BUOYANCY_POINT)
        for b in (1, 4):
            sl = slice(st["point_offset"][b], st["point_offset"][b] + st["point_count"][b])
            assert pts[sl].tobytes() == bytes(64 * st["point_count"][b])
        assert np.frombuffer(got["state"], W.RIGID_BODY)[[1, 4]].tobytes() == new.tobytes()
        gen.bodies_step(s, sc, 4, 1.0 / 120.0, {"warm_start": True})
        teleported[kernels] = gpu_arrays(gen, s)
        with pytest.raises(_lib.OceanWavesError) as e:   # the hull range is the body's own
            wrong = new[:1].copy()
            wrong["point_count"] += 1
            gen.bodies_set_state(s, wrong, first=1)
        assert e.value.status == _lib.OW_ERR_INVALID
        gen.bodies_destroy(s)
    assert outs["fused"] == outs["split"] == outs[None]
    assert teleported["fused"] == teleported["split"] == teleported[None]


@pytest.mark.gpu
def test_the_step_equals_the_host_loop_around_buoyancy_async(harness):
    """the loop of examples/buoyancy_host.c per substep: the pose record from the state (the CPU build), ow_buoyancy_async with the warm
    start, a synchronisation, the result read back, the CPU build of the integrator"""
    import torch
    n, ids = 512, [0, 1, 2]
    gen, params = gen_with(n, ids)
    sc = scales_of(params)
    st, hull = parity_scene()
    K, dt, opts = 6, 1.0 / 120.0, {"warm_start": True}
    s = gen.bodies_create(st, hull)
    gen.bodies_step(s, sc, K, dt, opts)
    got = gpu_arrays(gen, s)
    gen.bodies_destroy(s)

    state, flags = st.copy(), np.zeros(len(st), np.int32)
    dev = lambda x: torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).to("cuda:0")   # noqa: E731
    hull_dev = dev(hull)
    res_dev = torch.zeros(len(st) * 64, dtype=torch.uint8, device="cuda:0")
    pts_dev = torch.zeros(len(hull) * 64, dtype=torch.uint8, device="cuda:0")
    records = np.zeros(len(st), W.BUOYANCY_BODY)
    for _ in range(K):
        for b in range(len(st)):
            harness.harness_rigid_pose(state[b:b + 1].ctypes.data, records[b:b + 1].ctypes.data)
        gen.buoyancy_async(dev(records), hull_dev, sc, res_dev, pts_dev, opts)
        gen.sync()
        res = np.frombuffer(res_dev.cpu().numpy().tobytes(), W.BUOYANCY_RESULT).copy()
        for b in range(len(st)):
            harness.harness_rigid_finish(state[b:b + 1].ctypes.data, flags[b:b + 1].ctypes.data, res[b:b + 1].ctypes.data, dt, G32)
    assert got["state"] == state.tobytes()
    assert got["results"] == res.tobytes()
    assert got["points"] == pts_dev.cpu().numpy().tobytes()


def _ordering_case(stream=None, torch_stream=None):
    """update_all x 6, then the step with NO synchronisation in between, then more ticks: against a context that synchronises between the
    two calls (and stops there).  The step read the maps of exactly that point of the stream."""
    n, ids = 1024, [0, 1, 2, 3]
    a, pa = gen_with(n, ids, stream=stream, ticks=0)
    b, pb = gen_with(n, ids, ticks=0)
    sc = scales_of(pa)
    st, hull = demo_bodies(counts=(40, 64, 100, 16), seed=11)
    sa, sb = a.bodies_create(st, hull), b.bodies_create(st, hull)
    opts = {"warm_start": True}
    for _ in range(6):
        a.update_all(UPDATE_DELTA, pa)
    if torch_stream is not None:
        import torch
        with torch.cuda.stream(torch_stream):
            a.bodies_step(sa, sc, 4, 1.0 / 240.0, opts)
        rb, rr, rp = a.bodies_device_ptrs(sa)
        through = {"records": device_read(rb, sa.num_bodies, W.BUOYANCY_BODY, stream).tobytes(),
                   "results": device_read(rr, sa.num_bodies, W.BUOYANCY_RESULT, stream).tobytes(),
                   "points": device_read(rp, sa.num_points, W.BUOYANCY_POINT, stream).tobytes()}
    else:
        a.bodies_step(sa, sc, 4, 1.0 / 240.0, opts)
    for _ in range(6):
        a.update_all(UPDATE_DELTA, pa)
    got = gpu_arrays(a, sa)
    for _ in range(6):
        b.update_all(UPDATE_DELTA, pb)
    b.sync()
    b.bodies_step(sb, sc, 4, 1.0 / 240.0, opts)
    b.sync()
    want = gpu_arrays(b, sb)
    assert got == want
    if torch_stream is not None:
        for name in through:
            assert through[name] == want[name], name
    # the maps have moved since: the same step from the same start now gives other forces
    s2 = a.bodies_create(st, hull)
    a.bodies_step(s2, sc, 4, 1.0 / 240.0, opts)
    assert gpu_arrays(a, s2)["results"] != want["results"]
    assert a.bodies_stats(sa, faulted=False)["substeps"] == 4
    for g, s in ((a, sa), (a, s2), (b, sb)):
        g.bodies_destroy(s)
    return a


@pytest.mark.gpu
def test_the_step_is_ordered_behind_update_all_without_a_sync():
    a = _ordering_case()
    assert a.chain_stats() >= 0


@pytest.mark.gpu
def test_the_step_on_a_callers_stream():
    import torch
    s = torch.cuda.Stream()
    _ordering_case(stream=s.cuda_stream, torch_stream=s)


@pytest.mark.gpu
def test_faulted_layers_are_refused():
    """as ow_query_surface_async: once a synchronising call has reported a batch's device-side failure, its layers are refused (the
    project's own test hook makes a 2048^2 wave-pair rendezvous give up; the kernels run to completion)"""
    from godotoceanwaves_amd import WaveCascadeParameters
    from godotoceanwaves_amd.presets import cascade_preset
    gen = W()
    gen.map_size = 2048
    gen.init_gpu(2)
    params = [WaveCascadeParameters(**cascade_preset(1))]
    sc = scales_of(params)
    st, hull = demo_bodies(counts=(8, 8), seed=2)
    s = gen.bodies_create(st, hull)
    gen.update_all(UPDATE_DELTA, params)
    gen.sync()
    gen.bodies_step(s, sc, 2, 1.0 / 60.0)
    gen.debug_inject_fault(1)
    gen.update_all(UPDATE_DELTA, params)
    with pytest.raises(_lib.OceanWavesError):
        gen.sync()
    before = gen.bodies_stats(s, faulted=False)
    with pytest.raises(_lib.OceanWavesError) as e:
        gen.bodies_step(s, sc, 2, 1.0 / 60.0)
    assert e.value.status == _lib.OW_ERR_HIP
    assert gen.bodies_stats(s, faulted=False) == before   # nothing was enqueued
    gen.update_all(UPDATE_DELTA, params)                  # a clean batch recomputes the layer
    gen.bodies_step(s, sc, 2, 1.0 / 60.0)
    gen.sync()
    assert np.isfinite(gen.bodies_state(s)["position"]).all()
    gen.bodies_destroy(s)


@pytest.mark.gpu
def test_device_faults_are_counted_and_frozen(harness):
    n, ids = 256, [0, 1]
    gen, params = gen_with(n, ids)
    sc = scales_of(params)
    d, _ = gpu_maps(gen, len(ids))
    st, hull = make_bodies([crate(origin=(4.0 * i, 0.0, 0.0), divisions=(2, 2, 2)) for i in range(4)])
    st["linear_velocity"][2] = (0, 1.7e308, 0)   # passes the host's checks, overflows in its first substep
    st["mass"][3] = -1.0
    s = gen.bodies_create(st, hull)
    cs = CpuSet(harness, st, hull)
    gen.bodies_step(s, sc, 5, 10.0)
    cs.step(d, sc, 5, 10.0)
    assert gpu_arrays(gen, s) == cs.arrays()
    assert gen.bodies_stats(s)["faulted_bodies"] == 1 and list(cs.flags) == [0, 0, 1, 0]
    assert gen.bodies_state(s)[2].tobytes() == st[2].tobytes()
    fixed = st[2:3].copy()
    fixed["linear_velocity"] = 0.0
    gen.bodies_set_state(s, fixed, first=2)     # ... until its state is set again
    gen.bodies_step(s, sc, 5, 1.0 / 60.0)
    assert gen.bodies_stats(s)["faulted_bodies"] == 0 and gen.bodies_state(s)[2]["linear_velocity"][1] != 0.0
    gen.bodies_destroy(s)


@pytest.mark.gpu
def test_example_floats_its_crates_without_a_host_synchronisation(tmp_path):
    """256 crates of different sizes on the demo scene's three cascades, ow_update_all + one ow_bodies_step of 4 substeps per frame, the states
    and a stream-ordered history of pose and result records read back once at the end: finite; afloat per crate (its mean submerged share over
    time between a fifth and four fifths, its origin within 5 m of the water above it); nothing flagged by the device; no stream
    synchronisation by the library inside the loop (ow_sync_stats before and after)"""
    exe = build_example(tmp_path, "floating_bodies_host")
    r = subprocess.run([exe, "480"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert out["finite"] == "1" and out["afloat"] == "1" and out["host_syncs"] == "0" and out["faulted"] == "0", r.stdout
    assert int(out["bodies"]) >= 200 and int(out["snapshots"]) == 120 and int(out["substeps"]) == 4 * 480, r.stdout
    # per crate, over time: none sunk, none airborne (the smallest and the largest of the crates' mean submerged shares), none off the water
    assert 0.2 < float(out["share_min"]) <= float(out["submerged_share"]) <= float(out["share_max"]) < 0.8, r.stdout
    assert float(out["off_water_max"]) < 5.0, r.stdout


@pytest.mark.gpu
def test_a_set_that_outlives_its_context_is_orphaned_not_dangling():
    gen, params = gen_with(256, [0, 1])
    sc = scales_of(params)
    st, hull = demo_bodies(counts=(8, 8), seed=2)
    s = gen.bodies_create(st, hull)
    before = gen.sync_stats()
    gen.bodies_step(s, sc, 2, 1.0 / 60.0)
    assert gen.sync_stats() == before          # the step synchronises nothing
    gen.bodies_state(s)
    assert gen.sync_stats() == before + 1      # the read-back does
    handle = s.handle
    lib = gen._lib
    gen.free()                                  # the context goes first
    rec = np.zeros(1, W.RIGID_BODY)
    assert lib.ow_bodies_get_state(None, handle, 0, 1, rec.ctypes.data) == _lib.OW_ERR_INVALID
    lib.ow_bodies_destroy(None, handle)         # still the caller's to destroy; touches no freed memory


# ---- 14. cleanliness -------------------------------------------------------------------------------------------------------------------------

NEW_SOURCES = ("godotoceanwaves_amd/csrc/ow_rigid.h", "tests/bodies/bodies_harness.cpp", "tests/test_bodies_step.py", "examples/floating_bodies_host.c",
               "scripts/bench_bodies.py")


def test_new_sources_hold_none_of_the_forbidden_words_and_nothing_reads_the_reference():
    scalar = "s" + "_"
    words = [scalar + w for w in ("store" + "_dword", "buffer" + "_store", "scratch" + "_store", "atomic" + "_", "buffer" + "_atomic", "dcache" + "_wb",
                                  "dcache" + "_discard")]
    words += ["HSA_" + "XNACK", "xnack" + "+", "roc" + "gdb", "FORCE_GRAPH" + "_QUEUES"]
    for rel in NEW_SOURCES + ("godotoceanwaves_amd/csrc/ow_consumer.hip", "godotoceanwaves_amd/csrc/ow_runtime.hip"):
        text = open(os.path.join(ROOT, rel)).read().lower()
        for w in words:
            assert w.lower() not in text, (rel, w)
        assert "oracle/" + "_ref" not in text, rel
