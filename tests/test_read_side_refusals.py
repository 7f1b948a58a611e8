"""The read side's refusals, entry point by entry point, without a device: every entry point makes its argument checks before it touches
one, so a null context (or one bad argument) is answered with a status and an exact ow_last_error() text.  One table: what is called, with
what, and the text.  Where two faults are given at once the row pins which of them the caller hears about (the order of the checks); an
entry point with a synchronous and an `_async` form is called in both and has to give the same answer."""
import ctypes as C

import pytest

from godotoceanwaves_amd import _lib, build

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


class Args:
    """otherwise valid arguments, and the records with one fault each"""

    def __init__(self, lib):
        self.scales = (C.c_float * (4 * _lib.OW_MAX_CASCADES))(*([1.0] * (4 * _lib.OW_MAX_CASCADES)))
        self.xz = (C.c_float * 2)()
        self.origin = (C.c_float * 3)()
        self.buf = (C.c_char * 4096)()  # any non-null array: nothing is read or written behind a refusal
        self.out = C.c_void_p()
        self.u64 = C.c_uint64()
        self.cam = _lib.ow_camera(max_distance=100.0, basis=(C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), fov_y_degrees=60.0, width=4, height=4)
        self.cam0 = self.copy(self.cam, width=0)
        self.cam_reserved = self.copy(self.cam)
        self.cam_reserved.reserved[3] = 1
        self.verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 0, 1)
        self.idx = (C.c_int32 * 3)(0, 1, 2)
        self.idx_bad = (C.c_int32 * 3)(0, 1, 3)
        # options: the defaults, and one field wrong
        self.render = self.default(lib.ow_render_options_default, _lib.ow_render_options)
        self.render_rough = self.copy(self.render, roughness=2.0)
        self.render_iter = self.copy(self.render)
        self.render_iter.raycast.query.max_iterations = 65
        self.mesh = self.default(lib.ow_mesh_options_default, _lib.ow_mesh_options)
        self.mesh_lane = self.copy(self.mesh, lane_box=65)
        self.mesh_rough_near = self.copy(self.mesh, roughness=2.0, near=NAN)
        self.mesh_near = self.copy(self.mesh, near=NAN)
        self.spray = self.default(lib.ow_spray_options_default, _lib.ow_spray_options)
        self.spray_amount = self.copy(self.spray, amount=1)
        self.material = self.default(lib.ow_billboard_material_options_default, _lib.ow_billboard_material_options)
        self.material_alpha = self.copy(self.material, max_alpha=2.0)
        self.bins12 = _lib.ow_billboard_draw_options(bin_side=12)
        self.solid = self.default(lib.ow_solid_options_default, _lib.ow_solid_options)
        self.solid_flags = self.copy(self.solid, flags=2)
        self.solid_lane_flags = self.copy(self.solid, flags=2, lane_box=65)
        self.sky_srgb = self.copy(self.default(lib.ow_sky_options_default, _lib.ow_sky_options), srgb=2)
        self.env_fog = self.copy(self.default(lib.ow_environment_options_default, _lib.ow_environment_options), fog_mode=7)
        self.present = self.default(lib.ow_present_options_default, _lib.ow_present_options)
        self.present3 = self.copy(self.present, downsample=3)
        self.present5 = self.copy(self.present, downsample=5)
        self.radiance1 = self.copy(self.default(lib.ow_radiance_options_default, _lib.ow_radiance_options), levels=1)
        self.light_spec = self.copy(self.default(lib.ow_radiance_light_options_default, _lib.ow_radiance_light_options), specular=2.0)
        self.frame = self.default(lib.ow_shadow_frame_default, _lib.ow_shadow_frame)
        self.frame_dark = self.copy(self.frame, light_direction=(C.c_float * 3)(0, 0, 0))
        self.frame_flat = self.copy(self.frame, half_extent=0.0)
        self.taps4 = self.copy(self.default(lib.ow_shadow_options_default, _lib.ow_shadow_options), filter_taps=4)
        self.query65 = _lib.ow_query_options(max_iterations=65)
        self.buoy_warm = _lib.ow_buoyancy_options(flags=_lib.OW_BUOYANCY_WARM_START)
        self.buoy_iter = _lib.ow_buoyancy_options(query=self.query65)
        # 2 bodies x 2 hull points
        self.bodies2 = (_lib.ow_buoyancy_body * 2)()
        self.hull4 = (_lib.ow_hull_point * 4)()
        for b in range(2):
            self.bodies2[b].point_offset, self.bodies2[b].point_count = 2 * b, 2
        for i in range(4):
            self.hull4[i].volume, self.hull4[i].half_height, self.hull4[i].body = 1.0, 0.5, i // 2
        self.hull4_wrong = (_lib.ow_hull_point * 4).from_buffer_copy(self.hull4)
        self.hull4_wrong[1].body = 1
        self.rigid = _lib.ow_rigid_body(orientation=(C.c_double * 4)(0, 0, 0, 1), mass=1.0)
        self.rigid_q2 = self.copy(self.rigid, orientation=(C.c_double * 4)(0, 0, 0, 2))

    @staticmethod
    def default(fn, cls):
        o = cls()
        fn(C.byref(o))
        return o

    @staticmethod
    def copy(record, **fields):
        o = type(record).from_buffer_copy(record)
        for k, v in fields.items():
            setattr(o, k, v)
        return o


@pytest.fixture(scope="module")
def a(lib):
    return Args(lib)


R = C.byref
NULL_CONTEXT = "null context"

# (the entry point, or its two forms; a -> the arguments; the text).  The status is OW_ERR_INVALID in every row.
ROWS = [
    # ---- a null context behind otherwise valid arguments ----
    (("ow_sample_surface",), lambda a: (None, a.xz, 1, a.scales, 1, a.buf), NULL_CONTEXT),
    (("ow_query_surface", "ow_query_surface_async"), lambda a: (None, a.xz, 1, a.scales, 1, None, a.buf), NULL_CONTEXT),
    (("ow_query_velocity", "ow_query_velocity_async"), lambda a: (None, a.xz, 1, a.scales, 1, None, a.buf), NULL_CONTEXT),
    (("ow_raycast_surface", "ow_raycast_surface_async"), lambda a: (None, a.buf, 1, a.scales, 1, None, a.buf), NULL_CONTEXT),
    (("ow_update_velocity",), lambda a: (None, 1), NULL_CONTEXT),
    (("ow_get_velocity_ptrs",), lambda a: (None, R(a.out), None), NULL_CONTEXT),
    (("ow_get_velocity_map",), lambda a: (None, 0, a.buf), NULL_CONTEXT),
    (("ow_velocity_stats",), lambda a: (None, None, None), NULL_CONTEXT),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam), a.scales, 1, None, a.buf, None), NULL_CONTEXT),
    (("ow_buoyancy", "ow_buoyancy_async"), lambda a: (None, None, 0, None, 0, a.scales, 1, None, None, None), NULL_CONTEXT),
    (("ow_bodies_create",), lambda a: (None, R(a.rigid), 1, None, 0, R(a.out)), NULL_CONTEXT),
    (("ow_bodies_step",), lambda a: (None, None, a.scales, 1, None, 1, 0.01), NULL_CONTEXT),
    (("ow_bodies_get_state",), lambda a: (None, None, 0, 0, None), NULL_CONTEXT),
    (("ow_bodies_set_state",), lambda a: (None, None, 0, 0, None), NULL_CONTEXT),
    (("ow_bodies_get_results",), lambda a: (None, None, 0, 0, None), NULL_CONTEXT),
    (("ow_bodies_get_device_ptrs",), lambda a: (None, None, None, None, None), NULL_CONTEXT),
    (("ow_bodies_stats",), lambda a: (None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_sync_stats",), lambda a: (None, R(a.u64)), "null argument"),
    (("ow_mesh_create",), lambda a: (None, a.verts, 3, a.idx, 1, R(a.out)), NULL_CONTEXT),
    (("ow_mesh_displace",), lambda a: (None, None, a.origin, a.scales, 1, None, None, None), NULL_CONTEXT),
    (("ow_mesh_get_device_ptrs",), lambda a: (None, None, None, None), NULL_CONTEXT),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam), a.origin, a.scales, 1, None, a.buf, None), NULL_CONTEXT),
    (("ow_mesh_stats",), lambda a: (None, None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_spray_create",), lambda a: (None, R(a.spray), R(a.out)), NULL_CONTEXT),
    (("ow_spray_step",), lambda a: (None, None, 0.01, a.scales, 1), NULL_CONTEXT),
    (("ow_spray_read",), lambda a: (None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_spray_get_device_ptrs",), lambda a: (None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_spray_stats",), lambda a: (None, None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_billboard_material_create",), lambda a: (None, R(a.material), a.buf, 1, 1, a.buf, 1, 1, R(a.out)), NULL_CONTEXT),
    (("ow_billboard_draw", "ow_billboard_draw_async"), lambda a: (None, None, None, R(a.cam), None, a.buf, None), NULL_CONTEXT),
    (("ow_billboard_draw_instances",), lambda a: (None, None, None, 0, 0.0, R(a.cam), None, a.buf, None), NULL_CONTEXT),
    (("ow_billboard_draw_stats",), lambda a: (None, None, None, None, None), NULL_CONTEXT),
    (("ow_solid_create",), lambda a: (None, a.verts, 3, a.idx, 1, R(a.out)), NULL_CONTEXT),
    (("ow_solid_draw", "ow_solid_draw_async"), lambda a: (None, None, None, 0, 0, R(a.cam), None, a.buf, None), NULL_CONTEXT),
    (("ow_solid_draw_instances",), lambda a: (None, None, None, 0, R(a.cam), None, a.buf, None), NULL_CONTEXT),
    (("ow_solid_draw_stats",), lambda a: (None, None, None, None, None, None), NULL_CONTEXT),
    (("ow_sky_create",), lambda a: (None, None, a.buf, 1, 1, R(a.out)), NULL_CONTEXT),
    (("ow_environment_apply", "ow_environment_apply_async"), lambda a: (None, None, R(a.cam), None, a.buf), NULL_CONTEXT),
    (("ow_present", "ow_present_async"), lambda a: (None, R(a.cam), None, a.buf, a.buf, None), NULL_CONTEXT),
    (("ow_radiance_create",), lambda a: (None, None, None, R(a.out)), NULL_CONTEXT),
    (("ow_radiance_level",), lambda a: (None, None, 0, None, None, None, None), NULL_CONTEXT),
    (("ow_radiance_light_apply", "ow_radiance_light_apply_async"), lambda a: (None, None, R(a.cam), None, a.buf), NULL_CONTEXT),
    (("ow_shadow_map_create",), lambda a: (None, 8, R(a.out)), NULL_CONTEXT),
    (("ow_shadow_map_begin",), lambda a: (None, None, R(a.frame)), NULL_CONTEXT),
    (("ow_shadow_map_cast",), lambda a: (None, None, None, None, 0, 0), NULL_CONTEXT),
    (("ow_shadow_map_cast_instances",), lambda a: (None, None, None, None, 0), NULL_CONTEXT),
    (("ow_shadow_map_read",), lambda a: (None, None, a.buf), NULL_CONTEXT),
    (("ow_shadow_apply", "ow_shadow_apply_async"), lambda a: (None, None, R(a.cam), None, a.buf, None), NULL_CONTEXT),
    (("ow_shadow_stats",), lambda a: (None, None, None, None, None, None, None), NULL_CONTEXT),
    # ---- ow_render_view: the outputs, the scales, the camera, the options, the context ----
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam0), None, 1, R(a.render_rough), None, None), "null argument: both outputs"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam0), None, 1, R(a.render_rough), a.buf, None), "null argument"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, None, a.scales, 1, R(a.render_rough), a.buf, None), "null camera"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam0), a.scales, 1, R(a.render_rough), a.buf, None),
     "camera size 0 x 4 outside [1,8192]"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam_reserved), a.scales, 1, R(a.render_rough), a.buf, None),
     "ow_camera.reserved must be 0"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam), a.scales, 1, R(a.render_rough), a.buf, None), "roughness outside [0,1]"),
    (("ow_render_view", "ow_render_view_async"), lambda a: (None, R(a.cam), a.scales, 1, R(a.render_iter), None, a.buf),
     "max_iterations 65 outside [0,64]"),
    # ---- ow_mesh_draw: ow_render_view's order, the material before the draw's own fields, the context before the mesh and the origin ----
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, None, None, None, 1, R(a.mesh_lane), None, None), "null argument: both outputs"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam0), None, None, 1, R(a.mesh_lane), a.buf, None), "null argument"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam0), None, a.scales, 1, R(a.mesh_lane), a.buf, None),
     "camera size 0 x 4 outside [1,8192]"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam), None, a.scales, 1, R(a.mesh_rough_near), a.buf, None),
     "roughness outside [0,1]"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam), None, a.scales, 1, R(a.mesh_near), a.buf, None), "near is not finite"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam), None, a.scales, 1, R(a.mesh_lane), a.buf, None),
     "lane_box 65 outside [-1,64]"),
    (("ow_mesh_draw", "ow_mesh_draw_async"), lambda a: (None, None, R(a.cam), None, a.scales, 0, None, a.buf, None), NULL_CONTEXT),
    (("ow_mesh_displace",), lambda a: (None, None, None, None, 1, R(a.mesh_lane), R(a.cam_reserved), None), "null argument"),
    (("ow_mesh_displace",), lambda a: (None, None, None, a.scales, 1, R(a.mesh_lane), R(a.cam_reserved), None), "ow_camera.reserved must be 0"),
    (("ow_mesh_displace",), lambda a: (None, None, None, a.scales, 1, R(a.mesh_lane), R(a.cam0), None), "lane_box 65 outside [-1,64]"),
    (("ow_mesh_create",), lambda a: (None, a.verts, 0, None, 1, None), "null argument"),
    (("ow_mesh_create",), lambda a: (None, None, 0, None, 1, R(a.out)), "num_vertices and num_triangles must be >= 1"),
    (("ow_mesh_create",), lambda a: (None, a.verts, 3, a.idx_bad, 1, R(a.out)), "triangle 0: index 3 outside [0,3)"),
    # ---- ow_billboard_draw_instances: the count, the instances, the time, all before the camera ----
    (("ow_billboard_draw_instances",), lambda a: (None, None, None, -1, NAN, None, None, None, None), "count -1 outside [0,1048576]"),
    (("ow_billboard_draw_instances",), lambda a: (None, None, None, 1, NAN, None, None, None, None), "null argument"),
    (("ow_billboard_draw_instances",), lambda a: (None, None, a.buf, 1, NAN, None, None, None, None), "time is not finite"),
    (("ow_billboard_draw_instances",), lambda a: (None, None, a.buf, 1, 0.0, None, None, None, None), "null argument: both outputs"),
    (("ow_billboard_draw_instances",), lambda a: (None, None, a.buf, 1, 0.0, None, R(a.bins12), a.buf, None), "null camera"),
    (("ow_billboard_draw_instances",), lambda a: (None, None, a.buf, 1, 0.0, R(a.cam), R(a.bins12), a.buf, None),
     "bin_side 12 is not 0 or a multiple of 8 in [8,8192]"),
    (("ow_billboard_draw", "ow_billboard_draw_async"), lambda a: (None, None, None, None, R(a.bins12), None, None), "null argument: both outputs"),
    (("ow_billboard_draw", "ow_billboard_draw_async"), lambda a: (None, None, None, R(a.cam), R(a.bins12), None, a.buf),
     "bin_side 12 is not 0 or a multiple of 8 in [8,8192]"),
    (("ow_billboard_material_create",), lambda a: (None, None, a.buf, 1, 1, a.buf, 1, 1, R(a.out)), "null argument"),
    (("ow_billboard_material_create",), lambda a: (None, R(a.material_alpha), None, 0, 1, None, 1, 1, R(a.out)),
     "ow_billboard_material_options: max_alpha outside [0,1]"),
    (("ow_billboard_material_create",), lambda a: (None, R(a.material), None, 0, 1, None, 1, 1, R(a.out)), "texture side 0 outside [1,4096]"),
    (("ow_billboard_material_create",), lambda a: (None, R(a.material), None, 1, 1, a.buf, 1, 1, R(a.out)), "null argument"),
    # ---- the spray emitter ----
    (("ow_spray_create",), lambda a: (None, None, R(a.out)), "null argument"),
    (("ow_spray_create",), lambda a: (None, R(a.spray_amount), R(a.out)), "ow_spray_options: amount outside [4, 1048576]"),
    (("ow_spray_step",), lambda a: (None, None, 0.0, None, 9), "delta must be finite and > 0"),
    (("ow_spray_step",), lambda a: (None, None, 0.01, None, 9), "num_cascades 9 outside [1,8]"),
    (("ow_spray_step",), lambda a: (None, None, 0.01, None, 1), "null argument"),
    # ---- ow_solid_draw_instances: the count and the transforms before ow_billboard_draw's order ----
    (("ow_solid_draw_instances",), lambda a: (None, None, None, 65537, None, None, None, None), "count 65537 outside [0,65536]"),
    (("ow_solid_draw_instances",), lambda a: (None, None, None, 1, None, None, None, None), "null argument"),
    (("ow_solid_draw_instances",), lambda a: (None, None, a.buf, 1, None, R(a.solid_flags), None, None), "null argument: both outputs"),
    (("ow_solid_draw_instances",), lambda a: (None, None, a.buf, 1, None, R(a.solid_flags), a.buf, None), "null camera"),
    (("ow_solid_draw_instances",), lambda a: (None, None, a.buf, 1, R(a.cam), R(a.solid_lane_flags), a.buf, None), "lane_box 65 outside [-1,64]"),
    (("ow_solid_draw_instances",), lambda a: (None, None, a.buf, 1, R(a.cam), R(a.solid_flags), a.buf, None), "unknown solid flags 0x2"),
    (("ow_solid_draw", "ow_solid_draw_async"), lambda a: (None, None, None, -1, -1, R(a.cam0), R(a.solid_flags), None, None), "null argument: both outputs"),
    (("ow_solid_draw", "ow_solid_draw_async"), lambda a: (None, None, None, -1, -1, R(a.cam0), R(a.solid_flags), None, a.buf),
     "camera size 0 x 4 outside [1,8192]"),
    (("ow_solid_draw", "ow_solid_draw_async"), lambda a: (None, None, None, -1, -1, R(a.cam), R(a.solid_flags), None, a.buf), "unknown solid flags 0x2"),
    (("ow_solid_draw", "ow_solid_draw_async"), lambda a: (None, None, None, -1, -1, R(a.cam), None, None, a.buf), NULL_CONTEXT),
    (("ow_solid_create",), lambda a: (None, a.verts, 3, a.idx, 65537, R(a.out)), "num_vertices must be in [1,2^24] and num_triangles in [1,65536]"),
    (("ow_solid_create",), lambda a: (None, a.verts, 3, a.idx_bad, 1, R(a.out)), "triangle 0: index 3 outside [0,3)"),
    # ---- ow_environment_apply: the records, the camera, the options, the context ----
    (("ow_environment_apply", "ow_environment_apply_async"), lambda a: (None, None, None, R(a.env_fog), None), "null argument: the records"),
    (("ow_environment_apply", "ow_environment_apply_async"), lambda a: (None, None, None, R(a.env_fog), a.buf), "null camera"),
    (("ow_environment_apply", "ow_environment_apply_async"), lambda a: (None, None, R(a.cam), R(a.env_fog), a.buf), "unknown fog_mode 7"),
    (("ow_sky_create",), lambda a: (None, R(a.sky_srgb), None, 0, 1, None), "null argument"),
    (("ow_sky_create",), lambda a: (None, R(a.sky_srgb), None, 0, 1, R(a.out)), "panorama size 0 x 1 outside [1,8192]"),
    (("ow_sky_create",), lambda a: (None, R(a.sky_srgb), None, 1, 1, R(a.out)), "ow_sky_options: srgb is not 0 or 1"),
    (("ow_sky_create",), lambda a: (None, None, None, 1, 1, R(a.out)), "null argument"),
    # ---- ow_present: the outputs, the records, the camera, the options (a downsample that does not divide the size), the context ----
    (("ow_present", "ow_present_async"), lambda a: (None, None, R(a.present3), None, None, None), "null argument: both outputs"),
    (("ow_present", "ow_present_async"), lambda a: (None, None, R(a.present3), None, a.buf, None), "null argument: the records"),
    (("ow_present", "ow_present_async"), lambda a: (None, None, R(a.present3), a.buf, None, a.buf), "null camera"),
    (("ow_present", "ow_present_async"), lambda a: (None, R(a.cam), R(a.present3), a.buf, a.buf, None), "downsample 3 does not divide 4 x 4"),
    (("ow_present", "ow_present_async"), lambda a: (None, R(a.cam), R(a.present5), a.buf, a.buf, None), "downsample 5 outside [0,4]"),
    # ---- the radiance pyramid and its pass: ow_environment_apply's order ----
    (("ow_radiance_create",), lambda a: (None, None, R(a.radiance1), None), "null argument"),
    (("ow_radiance_create",), lambda a: (None, None, R(a.radiance1), R(a.out)), "ow_radiance_options: levels 1 outside [2,8]"),
    (("ow_radiance_light_apply", "ow_radiance_light_apply_async"), lambda a: (None, None, None, R(a.light_spec), None), "null argument: the records"),
    (("ow_radiance_light_apply", "ow_radiance_light_apply_async"), lambda a: (None, None, R(a.cam0), R(a.light_spec), a.buf),
     "camera size 0 x 4 outside [1,8192]"),
    (("ow_radiance_light_apply", "ow_radiance_light_apply_async"), lambda a: (None, None, R(a.cam), R(a.light_spec), a.buf),
     "ow_radiance_light_options: specular outside [0,1]"),
    # ---- the sun shadows ----
    (("ow_shadow_map_create",), lambda a: (None, 4, None), "null argument"),
    (("ow_shadow_map_create",), lambda a: (None, 4, R(a.out)), "shadow map size 4 outside [8,8192]"),
    (("ow_shadow_map_begin",), lambda a: (None, None, None), "null frame"),
    (("ow_shadow_map_begin",), lambda a: (None, None, R(a.frame_flat)), "ow_shadow_frame: half_extent outside (0,1e6]"),
    (("ow_shadow_map_begin",), lambda a: (None, None, R(a.frame_dark)), "light_direction has zero length"),
    (("ow_shadow_map_cast_instances",), lambda a: (None, None, None, None, -1), "count -1 outside [0,65536]"),
    (("ow_shadow_map_cast_instances",), lambda a: (None, None, None, None, 1), "null argument"),
    (("ow_shadow_map_read",), lambda a: (None, None, None), "null argument"),
    (("ow_shadow_apply", "ow_shadow_apply_async"), lambda a: (None, None, None, R(a.taps4), None, None), "null argument: the records"),
    (("ow_shadow_apply", "ow_shadow_apply_async"), lambda a: (None, None, None, R(a.taps4), a.buf, None), "null camera"),
    (("ow_shadow_apply", "ow_shadow_apply_async"), lambda a: (None, None, R(a.cam), R(a.taps4), a.buf, None),
     "filter_taps 4 is not one of 0, 1, 3, 5, 7, 9"),
    # ---- ow_buoyancy: counts, options, pointers, (the host form) the arrays themselves, the context ----
    (("ow_buoyancy", "ow_buoyancy_async"), lambda a: (None, None, -1, None, 0, None, 1, R(a.buoy_iter), None, None),
     "num_bodies and num_points must be >= 0"),
    (("ow_buoyancy", "ow_buoyancy_async"), lambda a: (None, None, 2, None, 4, None, 1, R(a.buoy_iter), None, None), "max_iterations 65 outside [0,64]"),
    (("ow_buoyancy", "ow_buoyancy_async"), lambda a: (None, None, 2, None, 4, None, 1, R(a.buoy_warm), None, None), "null argument"),
    (("ow_buoyancy",), lambda a: (None, a.bodies2, 2, a.hull4_wrong, 4, a.scales, 1, R(a.buoy_warm), a.buf, None),
     "OW_BUOYANCY_WARM_START needs points_inout"),
    (("ow_buoyancy_async",), lambda a: (None, a.bodies2, 2, a.hull4_wrong, 4, a.scales, 1, R(a.buoy_warm), a.buf, None), "points_dev is required"),
    (("ow_buoyancy",), lambda a: (None, a.bodies2, 2, a.hull4_wrong, 4, a.scales, 1, None, a.buf, None),
     "hull point 1 lies in body 0's range but names body 1"),
    (("ow_buoyancy",), lambda a: (None, a.bodies2, 2, a.hull4, 4, a.scales, 1, None, a.buf, None), NULL_CONTEXT),
    (("ow_buoyancy_async",), lambda a: (None, a.bodies2, 2, a.hull4_wrong, 4, a.scales, 1, None, a.buf, a.buf), NULL_CONTEXT),  # device arrays are not read
    # ---- the floating bodies ----
    (("ow_bodies_create",), lambda a: (None, R(a.rigid_q2), 1, None, 0, None), "null argument"),
    (("ow_bodies_create",), lambda a: (None, R(a.rigid_q2), 0, None, 0, R(a.out)), "num_bodies must be >= 1 and num_points >= 0"),
    (("ow_bodies_create",), lambda a: (None, R(a.rigid_q2), 1, None, 0, R(a.out)), "body 0: orientation must be a unit quaternion (|q| = 2)"),
    (("ow_bodies_step",), lambda a: (None, None, None, 1, None, 0, 0.0), "substeps 0 outside [1,64]"),
    (("ow_bodies_step",), lambda a: (None, None, None, 1, None, 1, 0.0), "dt must be finite and > 0"),
    (("ow_bodies_step",), lambda a: (None, None, None, 1, None, 1, 0.01), "null argument"),
    (("ow_sync_stats",), lambda a: (None, None), "null argument"),
    # ---- the point calls look at the context first: its cascade count bounds num_cascades ----
    (("ow_query_surface", "ow_query_surface_async"), lambda a: (None, None, -1, None, 0, R(a.query65), None), NULL_CONTEXT),
    (("ow_query_velocity", "ow_query_velocity_async"), lambda a: (None, None, -1, None, 0, R(a.query65), None), NULL_CONTEXT),
    (("ow_raycast_surface", "ow_raycast_surface_async"), lambda a: (None, None, -1, None, 0, None, None), NULL_CONTEXT),
    (("ow_get_velocity_ptrs",), lambda a: (None, None, None), NULL_CONTEXT),
    (("ow_get_velocity_map",), lambda a: (None, -1, None), NULL_CONTEXT),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=[f"{i}-{r[0][0]}" for i, r in enumerate(ROWS)])
def test_refusal(lib, a, row):
    names, args, text = ROWS[row]
    answers = []
    for name in names:
        status = getattr(lib, name)(*args(a))
        answers.append((status, lib.ow_last_error().decode()))
    assert answers == [(_lib.OW_ERR_INVALID, text)] * len(names)


def test_every_moved_entry_point_with_a_context_has_a_null_context_row():
    covered = {n for names, _, text in ROWS for n in names if text == NULL_CONTEXT or n == "ow_sync_stats"}  # ow_sync_stats: "null argument"
    prefixes = ("ow_sample_surface", "ow_query_", "ow_raycast_", "ow_buoyancy", "ow_bodies_", "ow_sync_stats", "ow_update_velocity", "ow_get_velocity_",
                "ow_velocity_stats", "ow_render_view", "ow_mesh_", "ow_spray_", "ow_billboard_", "ow_solid_", "ow_sky_", "ow_environment_",
                "ow_present", "ow_radiance_", "ow_shadow_")
    moved = {n for n in _lib.SIGNATURES if n.startswith(prefixes) and not n.endswith(("_default", "_destroy")) and n != "ow_query_link"}
    assert moved <= covered, sorted(moved - covered)


def test_defaults_and_destroys_take_null(lib):
    defaults = [n for n in _lib.SIGNATURES if n.endswith("_default") and n != "ow_cascade_params_default"]
    assert len(defaults) == 12
    for name in defaults:
        getattr(lib, name)(None)  # returns without writing
    destroys = [n for n in _lib.SIGNATURES if n.endswith("_destroy") and n not in ("ow_destroy", "ow_group_destroy")]
    assert len(destroys) == 8
    for name in destroys:
        getattr(lib, name)(None, None)  # no handle: nothing to do, and the context is not looked at
