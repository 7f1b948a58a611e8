"""The inputs of tests/test_written_maps_gpu.py, checked on the CPU builds and in plain NumPy before a device is involved
(tests/device_maps.py builds them): every finite FP16 pattern comes back from a sample at its texel's centre, and the last column takes
load_quad's wrap branch; every spike case of the height bound gives the slab of ow_raycast.h's formula and other records than the same
map without the spike, so a slab that is too thin shows; the non-finite heights give the whole ray; the zero maps at the device's
smallest size are the analytic calm sea."""
import numpy as np
import pytest

from checks import calm_plane, check_calm_hits, check_calm_misses, check_picture, check_texel_centres
from cpu_builds import cpu_mesh_draw, cpu_raycast, cpu_render, cpu_sample
from cpu_builds import mesh_harness, query_harness, raycast_harness, render_harness  # noqa: F401 (fixtures)
from device_maps import (bound_cases, BOUND_SIZES, DISP_REPORTED, FINITE_PATTERNS, FP16_N, fp16_layout, FP16_SCALES, NON_FINITE, non_finite_case,
                         NORM_REPORTED, texel_points)
from scenes import CALM_CAMERAS, calm_hit_rays, calm_maps, calm_miss_rays, grid_with_a_fan, HIT, INVALID, look, NEAR

FINITE = np.array([p for p in range(65536) if (p & 0x7c00) != 0x7c00], np.uint16)


# ---- A. every finite FP16 value ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_every_finite_pattern_comes_back_exactly_from_its_texels_centre(query_harness, reverse):
    d, m = fp16_layout(reverse)
    assert len(FINITE) == FINITE_PATTERNS == 63488
    for layer in (d, m):
        assert not ((layer & 0x7c00) == 0x7c00).any()
    assert np.isin(FINITE, np.union1d(d[..., DISP_REPORTED], m[..., NORM_REPORTED])).all()      # ... in a half-word that a record reports
    xz = texel_points(0.5)
    uv = xz * FP16_SCALES[0, :2]
    taps, weights = np.zeros((len(xz), 4), np.int32), np.zeros((len(xz), 2), np.float32)
    query_harness.harness_tap(uv.ctypes.data, len(uv), FP16_N, taps.ctypes.data, weights.ctypes.data)
    rows, cols = np.divmod(np.arange(len(xz)), FP16_N)
    assert not weights.any() and np.array_equal(taps[:, 0], rows) and np.array_equal(taps[:, 2], cols)
    wraps = taps[:, 3] != taps[:, 2] + 1
    assert np.array_equal(wraps, cols == FP16_N - 1) and wraps.sum() == FP16_N        # column 127: two 8-byte loads a row on the device
    exact = check_texel_centres(cpu_sample(query_harness, d, m, FP16_SCALES, xz), d, m)
    assert np.isin(FINITE, exact).all() and len(exact) == FINITE_PATTERNS
    # the other layout puts other values on the last column and row
    od, _ = fp16_layout(not reverse)
    assert not np.array_equal(np.sort(d[0, :, -1].ravel()), np.sort(od[0, :, -1].ravel()))
    assert not np.array_equal(np.sort(d[0, -1].ravel()), np.sort(od[0, -1].ravel()))


def test_the_corner_points_give_all_four_taps_a_weight(query_harness):
    xz = texel_points(1.0)
    uv = xz * FP16_SCALES[0, :2]
    taps, weights = np.zeros((len(xz), 4), np.int32), np.zeros((len(xz), 2), np.float32)
    query_harness.harness_tap(uv.ctypes.data, len(uv), FP16_N, taps.ctypes.data, weights.ctypes.data)
    assert (weights == 0.5).all() and (taps[:, 3] != taps[:, 2] + 1).sum() == FP16_N
    for reverse in (False, True):
        d, m = fp16_layout(reverse)
        out = cpu_sample(query_harness, d, m, FP16_SCALES, xz)
        for f in ("displacement", "gradient", "foam", "gradient_fragment", "foam_fragment"):
            assert np.isfinite(out[f]).all(), f        # finite texels, weights that sum to 1: the records are finite and hold no NaN to compare


# ---- B. the height bound ---------------------------------------------------------------------------------------------------------------------

def differ(a, b):
    """per record: does any field differ"""
    flat = lambda r: np.frombuffer(r.tobytes(), np.uint8).reshape(r.size, -1)   # noqa: E731
    return (flat(a) != flat(b)).any(axis=1)


@pytest.mark.parametrize("n", BOUND_SIZES)
def test_every_spike_case_has_the_formulas_slab_and_shows_a_wrong_bound(raycast_harness, render_harness, n):
    """per case: slab_half_height is ow_raycast.h's formula on the known maxima; the ray straight down on each spike lands on its top;
    and the same map without a spike -- the map a bound that missed the spike stands for -- gives other records for at least one ray
    (in its status or t, not only in the slab it reports) and for at least one pixel"""
    for case in bound_cases(n):
        d, m = case.maps()
        rays, cam, sc = case.rays(), case.camera(), case.scales
        out = cpu_raycast(raycast_harness, d, m, sc, rays)
        assert len(rays) == 12 and not (out["status"] & INVALID).any(), case.name
        assert (out["slab_half_height"] == case.slab()).all() and case.slab() > np.float32(0.01), (case.name, out["slab_half_height"][0], case.slab())
        per = len(rays) // len(case.spikes)
        for k in range(len(case.spikes)):
            first = out[k * per]
            assert first["status"] == HIT and abs(first["position"][1] - case.world(k)[2]) <= 5e-3, (case.name, k, first["position"])
            d0, m0 = case.maps(without=(k,))
            out0 = cpu_raycast(raycast_harness, d0, m0, sc, rays)
            assert differ(out, out0).any() and ((out["status"] != out0["status"]) | (out["t"] != out0["t"])).any(), (case.name, k)
        _, rec = cpu_render(render_harness, d, m, sc, cam)
        d0, m0 = case.maps(without=tuple(range(len(case.spikes))))
        _, rec0 = cpu_render(render_harness, d0, m0, sc, cam)
        assert ((rec["status"] & HIT) != 0).all() and differ(rec, rec0).any(), case.name


@pytest.mark.parametrize("bits", NON_FINITE, ids=[f"{b:#06x}" for b in NON_FINITE])
def test_a_non_finite_height_makes_the_slab_the_whole_ray(raycast_harness, bits):
    case = non_finite_case(bits)
    d, m = case.maps()
    assert case.slab() == np.float32(3.4028235e38)
    out = cpu_raycast(raycast_harness, d, m, case.scales, case.rays(), case.options)
    assert (out["slab_half_height"] == np.float32(3.4028235e38)).all() and (out["samples"] > 0).all()
    assert (out["rounds"] <= 1 + 4).all() and (out["samples"] <= 64 + 4 * 63).all()      # one march round of max_samples, four of refinement
    for f in out.dtype.names:
        if out[f].dtype.kind == "f":
            assert np.isfinite(out[f]).all(), f        # the rays stay away from the texel: no NaN whose bits two builds could write differently
    assert np.isfinite(out["query"]["sample"]["displacement"]).all() and ((out["status"] & HIT) != 0).any()


def test_zero_maps_at_128_are_the_calm_sea(raycast_harness):
    d, m, sc = calm_maps(128)
    rays, h = calm_hit_rays(1.25)
    check_calm_hits(cpu_raycast(raycast_harness, d, m, sc, rays, {"water_level": 1.25}), rays, h)
    check_calm_misses(cpu_raycast(raycast_harness, d, m, sc, calm_miss_rays(-0.5), {"water_level": -0.5, "max_samples": 64}), -0.5)


# ---- C. a calm sea drawn -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CALM_CAMERAS))
def test_zero_maps_at_128_draw_the_analytic_plane(mesh_harness, name):
    d, m, sc = calm_maps(128)
    kw, opts = CALM_CAMERAS[name]
    cam = look(width=64, height=40, **kw)
    mesh = grid_with_a_fan()
    pic = cpu_mesh_draw(mesh_harness, d, m, sc, mesh, (0, 0, 0), cam, opts)
    hit = check_picture(pic, len(mesh[1]), opts)
    _, _, asked, want = calm_plane(cam, opts.get("near", NEAR))
    assert np.array_equal(hit[asked], want[asked]) and want.any() and asked.mean() > 0.98
