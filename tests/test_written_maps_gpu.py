"""The read side's device-only code on maps a test wrote (tests/device_maps.py: a context over caller-owned buffers, never ticked), held to
the CPU builds bit for bit, field by field, and to values known exactly.  tests/test_written_maps.py checks the same inputs on the CPU
builds alone.

What this reaches that generated maps do not: the device branch of load_quad (ow_surface.h: 16-byte loads, __builtin_convertvector from
_Float16, the wrap branch of the last column) on every finite FP16 pattern; k_height_bound (ow_consumer.hip) with the maximum in the first
and the last texel pair, in the odd texel of a pair, at the seam between the grid-stride loop's trips, in each cascade, with a zero and
with a non-finite bound, from ow_raycast_surface and from ow_render_view; and a calm sea drawn and rendered on the device."""
import numpy as np
import pytest

from checks import (assert_same_image, assert_same_picture, assert_same_records, calm_plane, check_calm_hits, check_calm_misses, check_picture,
                    check_texel_centres)
from cpu_builds import cpu_mesh_draw, cpu_raycast, cpu_render, cpu_sample
from cpu_builds import mesh_harness, query_harness, raycast_harness, render_harness  # noqa: F401 (fixtures)
from device_maps import (bound_cases, BOUND_SIZES, FP16_N, fp16_layout, FP16_SCALES, NON_FINITE, non_finite_case, texel_points, written_context)
from scenes import (CALM_CAMERAS, calm_hit_rays, calm_maps, calm_miss_rays, gpu_mesh_draw, grid_with_a_fan, HIT, INVALID, look, NEAR, swell_maps,
                    swell_rays)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    """one written context per (map size, cascades), made on first use and shared: no test ticks one"""
    made = {}

    def get(n, cascades):
        if (n, cascades) not in made:
            made[n, cascades] = written_context(n, cascades)
        return made[n, cascades]
    yield get
    for ctx in made.values():
        ctx.free()


# ---- A. every finite FP16 value through the device's loads -----------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_every_finite_pattern_through_the_device_loads(query_harness, contexts, reverse):
    ctx = contexts(FP16_N, 1)
    d, m = ctx.write(*fp16_layout(reverse))
    centres, corners = texel_points(0.5), texel_points(1.0)
    got = ctx.gen.sample_surface(centres, FP16_SCALES)
    check_texel_centres(got, d, m)
    assert_same_records(got, cpu_sample(query_harness, d, m, FP16_SCALES, centres), "texel centres")
    assert_same_records(ctx.gen.sample_surface(corners, FP16_SCALES), cpu_sample(query_harness, d, m, FP16_SCALES, corners), "texel corners")


# ---- B. the height bound, position by position ---------------------------------------------------------------------------------------------

def cast(ctx, raycast_harness, case):
    """the case's rays on the device: the slab of the formula on the known maxima, and the CPU build's records; returns the maps written"""
    d, m = ctx.write(*case.maps())
    rays, sc = case.rays(), case.scales
    got = ctx.gen.raycast_surface(rays, sc, case.options)
    assert not (got["status"] & INVALID).any() and (got["slab_half_height"] == case.slab()).all(), (case.name, got["slab_half_height"], case.slab())
    assert_same_records(got, cpu_raycast(raycast_harness, d, m, sc, rays, case.options), case.name)
    return d, m


@pytest.mark.parametrize("n", BOUND_SIZES)
def test_the_height_bound_finds_a_spike_wherever_it_is(raycast_harness, render_harness, contexts, n):
    ctx = contexts(n, 3)
    for case in bound_cases(n):
        d, m = cast(ctx, raycast_harness, case)
        cam = case.camera()
        assert_same_image(ctx.gen.render_view(cam, case.scales), cpu_render(render_harness, d, m, case.scales, cam), case.name)


@pytest.mark.parametrize("bits", NON_FINITE, ids=[f"{b:#06x}" for b in NON_FINITE])
def test_a_non_finite_height_makes_the_slab_the_whole_ray(raycast_harness, contexts, bits):
    case = non_finite_case(bits)
    d, m = case.maps()
    want = cpu_raycast(raycast_harness, d, m, case.scales, case.rays(), case.options)      # first: every march ends within max_samples
    assert (want["slab_half_height"] == np.float32(3.4028235e38)).all() and (want["rounds"] <= 1 + 4).all()
    cast(contexts(case.n, 3), raycast_harness, case)


def test_zero_maps_give_the_slabs_floor_and_the_analytic_hits(raycast_harness, contexts):
    ctx = contexts(128, 2)
    d, m, sc = calm_maps(128)
    ctx.write(d, m)
    rays, h = calm_hit_rays(1.25)
    got = ctx.gen.raycast_surface(rays, sc, {"water_level": 1.25})
    assert (got["slab_half_height"] == np.float32(0.01)).all()
    check_calm_hits(got, rays, h)
    assert_same_records(got, cpu_raycast(raycast_harness, d, m, sc, rays, {"water_level": 1.25}), "calm hits")
    opts = {"water_level": -0.5, "max_samples": 64}
    got = ctx.gen.raycast_surface(calm_miss_rays(-0.5), sc, opts)
    check_calm_misses(got, -0.5)
    assert_same_records(got, cpu_raycast(raycast_harness, d, m, sc, calm_miss_rays(-0.5), opts), "calm misses")


def test_the_swell_field_bit_for_bit(raycast_harness, contexts):
    d, m, sc = swell_maps()
    ctx = contexts(d.shape[1], 1)
    ctx.write(d, m)
    rays = swell_rays()
    got = ctx.gen.raycast_surface(rays, sc)
    assert ((got["status"] & HIT) != 0).all()
    assert_same_records(got, cpu_raycast(raycast_harness, d, m, sc, rays), "swell")


# ---- C. a calm sea drawn on the device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CALM_CAMERAS))
def test_a_calm_sea_drawn_and_rendered_on_the_device(mesh_harness, render_harness, contexts, name):
    ctx = contexts(128, 2)
    d, m, sc = calm_maps(128)
    ctx.write(d, m)
    kw, opts = CALM_CAMERAS[name]
    cam = look(width=64, height=40, **kw)
    mesh = grid_with_a_fan()
    handle = ctx.gen.mesh_create(*mesh)
    got = gpu_mesh_draw(ctx.gen, handle, cam, (0, 0, 0), sc, opts)
    ctx.gen.mesh_destroy(handle)
    assert_same_picture(got, cpu_mesh_draw(mesh_harness, d, m, sc, mesh, (0, 0, 0), cam, opts), name)
    hit = check_picture(got, len(mesh[1]), opts)
    _, _, asked, want = calm_plane(cam, opts.get("near", NEAR))
    assert np.array_equal(hit[asked], want[asked]) and want.any() and asked.mean() > 0.98
    assert_same_image(ctx.gen.render_view(cam, sc), cpu_render(render_harness, d, m, sc, cam), name)
