"""ctypes binding of include/ocean_waves.h (libocean_waves.so).  Fails loudly: no fallback of any kind."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OCEAN_WAVES_LIB: developer override to A/B a differently built library (scripts/build_variant.sh); same loud failure if missing
LIB_PATH = os.environ.get("OCEAN_WAVES_LIB") or os.path.join(_HERE, "libocean_waves.so")

OW_MAX_CASCADES = 8
OW_MAX_DEVICES = 8
OW_GROUP_FLAG_FORCE_PEER_PATH = 0x10000
OW_FLAG_DEBUG_F32 = 1
OW_FLAG_KERNELS_STANDARD = 2
OW_FLAG_KERNELS_LAYER_PARALLEL = 4
OW_FLAG_KERNELS_COMPACT = 8
OW_FLAG_NO_TICK_GROUPS = 16
OW_FLAG_RUN_AS_CALLS = 32
OW_FLAG_RUN_AS_REFERENCE_SCHEDULE = 64
OW_FLAG_GROUP_P1_LP, OW_FLAG_GROUP_P1_COMPACT, OW_FLAG_GROUP_P2_PLAIN, OW_FLAG_GROUP_P2_PIPE = 0x100, 0x200, 0x400, 0x800
OW_FLAG_ALWAYS_REGENERATE_SPECTRUM = 0x1000
OW_FLAG_LAZY_SCRATCH = 0x2000
OW_FLAG_SINGLE_STREAM = 0x4000
OW_FLAG_BODIES_FUSED, OW_FLAG_BODIES_SPLIT = 0x8000, 0x20000
OW_BODIES_MAX_SUBSTEPS = 64
OW_QUERY_DISTANCE_FALLOFF = 1
OW_BUOYANCY_WARM_START = 1
OW_BUOYANCY_WATER_VELOCITY = 2
OW_RAY_HIT, OW_RAY_FROM_BELOW, OW_RAY_TRUNCATED, OW_RAY_INVALID = 1, 2, 4, 8
OW_RAY_SOLID = 16
OW_SOLID_TWO_SIDED = 1
OW_SOLID_MAX_INSTANCES, OW_SOLID_MAX_TRIANGLES = 65536, 65536
OW_SOLID_CAST_TWO_SIDED = 1
OW_RAY_ENVIRONMENT = 32
OW_RAY_SKY_LIT = 64
OW_RADIANCE_MAX_LEVELS, OW_RADIANCE_MAX_SAMPLES, OW_RADIANCE_IRRADIANCE = 8, 256, -1
OW_RAY_SHADOWED = 128
OW_SHADOW_CAST_BOTH_SIDES, OW_SHADOW_RECEIVE_WATER = 1, 1
OW_SHADOW_MIN_SIZE, OW_SHADOW_MAX_SIZE = 8, 8192
OW_RAY_MIST = 256
OW_MIST_MAX_SLICES = 256
OW_RAY_MIRROR = 512
OW_MIRROR_TWO_SIDED = 1
OW_SKY_MAX_SIDE = 8192
OW_PRESENT_MAX_DOWNSAMPLE = 4
OW_FOG_EXPONENTIAL, OW_FOG_DEPTH = 0, 1
OW_TONEMAP_LINEAR, OW_TONEMAP_REINHARD, OW_TONEMAP_FILMIC = 0, 1, 2
OW_RENDER_MAX_SIDE = 8192
OW_MESH_CULL_BACK = 1
OW_MESH_VERTEX_NOT_FINITE = 1
OW_SPRAY_ACTIVE, OW_SPRAY_HAS_STARTED, OW_SPRAY_RESTARTED = 1, 2, 4
OW_SPRAY_MIN_AMOUNT, OW_SPRAY_MAX_AMOUNT = 4, 1048576
OW_BILLBOARD_TEXTURE_MAX_SIDE = 4096
OW_OK, OW_ERR_INVALID, OW_ERR_NO_DEVICE, OW_ERR_HIP, OW_ERR_NOMEM, OW_ERR_STATE = range(6)


class OceanWavesError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"ocean_waves status {status}: {message}")
        self.status = status


class ow_cascade_params(C.Structure):
    """struct ow_cascade_params (WaveCascadeParameters, wave_cascade_parameters.gd:7-42), ABI 4: the scalar parameters are FP64 as a
    GDScript caller holds them (the library narrows where the reference does); tile_length is a Vector2 (FP32 components)"""
    _fields_ = [("tile_length", C.c_float * 2), ("displacement_scale", C.c_double), ("normal_scale", C.c_double),
                ("wind_speed", C.c_double), ("wind_direction", C.c_double), ("fetch_length", C.c_double),
                ("swell", C.c_double), ("spread", C.c_double), ("detail", C.c_double), ("whitecap", C.c_double),
                ("foam_amount", C.c_double), ("spectrum_seed", C.c_int32 * 2),
                ("should_generate_spectrum", C.c_int32), ("reserved", C.c_int32), ("time", C.c_double),
                ("foam_grow_rate", C.c_double), ("foam_decay_rate", C.c_double)]


class ow_push_constants(C.Structure):
    """the reference's three push-constant blocks of one cascade, as 32-bit words (ow_get_push_constants)"""
    _fields_ = [("spectrum", C.c_uint32 * 16), ("modulate", C.c_uint32 * 8), ("unpack", C.c_uint32 * 4)]


class ow_config(C.Structure):
    _fields_ = [("map_size", C.c_int32), ("num_cascades", C.c_int32), ("device_id", C.c_int32), ("depth", C.c_float),
                ("stream", C.c_void_p), ("displacement_map", C.c_void_p), ("normal_map", C.c_void_p),
                ("flags", C.c_uint32)]


class ow_group_config(C.Structure):
    _fields_ = [("map_size", C.c_int32), ("num_devices", C.c_int32), ("device_ids", C.c_int32 * OW_MAX_DEVICES),
                ("cascades_per_device", C.c_int32), ("root", C.c_int32), ("depth", C.c_float), ("flags", C.c_uint32),
                ("displacement_map", C.c_void_p), ("normal_map", C.c_void_p)]


class ow_group_link(C.Structure):
    """how a shard's layers reach the root device (ow_group_link_info / ow_query_link)"""
    _fields_ = [("device", C.c_int32), ("root_device", C.c_int32), ("same_device", C.c_int32), ("peer_access", C.c_int32),
                ("link_type", C.c_int32), ("hops", C.c_int32), ("staged_path", C.c_int32), ("reserved", C.c_int32)]

    LINK_TYPES = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi", -1: "unknown"}

    def as_dict(self):
        return {"device": self.device, "root_device": self.root_device, "same_device": bool(self.same_device), "peer_access": bool(self.peer_access),
                "link": self.LINK_TYPES.get(self.link_type, str(self.link_type)), "hops": self.hops, "staged_path": bool(self.staged_path)}


class ow_surface_sample(C.Structure):
    """struct ow_surface_sample (64 bytes): what the water / spray shaders read at a world point"""
    _fields_ = [("displacement", C.c_float * 3), ("gradient", C.c_float * 2), ("gradient_scaled", C.c_float * 2), ("foam", C.c_float),
                ("normal_factor", C.c_float), ("foam_factor", C.c_float), ("scale_factor", C.c_float), ("spray_active", C.c_int32),
                ("gradient_fragment", C.c_float * 2), ("foam_fragment", C.c_float), ("reserved", C.c_float)]


class ow_query_options(C.Structure):
    """struct ow_query_options (32 bytes); zeros = the defaults (16 iterations, 1e-3 m, no distance falloff)"""
    _fields_ = [("max_iterations", C.c_int32), ("tolerance", C.c_float), ("flags", C.c_uint32), ("falloff_center_xz", C.c_float * 2),
                ("reserved", C.c_uint32 * 3)]


class ow_surface_query(C.Structure):
    """struct ow_surface_query (128 bytes): the water above a world point, ow_surface_sample embedded at offset 64"""
    _fields_ = [("p", C.c_float * 2), ("residual", C.c_float), ("iterations", C.c_int32), ("evaluations", C.c_int32),
                ("converged", C.c_int32), ("falloff", C.c_float), ("height", C.c_float), ("normal", C.c_float * 3),
                ("world_xz", C.c_float * 2), ("reserved", C.c_int32 * 3), ("sample", ow_surface_sample)]


class ow_surface_velocity(C.Structure):
    """struct ow_surface_velocity (32 bytes): the velocity of the rendered surface above a world point, with the query's height and p"""
    _fields_ = [("velocity", C.c_float * 3), ("height", C.c_float), ("p", C.c_float * 2), ("converged", C.c_int32), ("reserved", C.c_uint32)]


class ow_buoyancy_body(C.Structure):
    """struct ow_buoyancy_body (96 bytes): a pose in Godot's Transform3D layout (basis rows, then origin), velocities, the hull range, drag"""
    _fields_ = [("transform", C.c_float * 12), ("linear_velocity", C.c_float * 3), ("angular_velocity", C.c_float * 3),
                ("point_offset", C.c_int32), ("point_count", C.c_int32), ("linear_drag", C.c_float), ("quadratic_drag", C.c_float),
                ("reserved", C.c_uint32 * 2)]


class ow_hull_point(C.Structure):
    """struct ow_hull_point (32 bytes)"""
    _fields_ = [("local", C.c_float * 3), ("volume", C.c_float), ("half_height", C.c_float), ("body", C.c_int32), ("reserved", C.c_uint32 * 2)]


class ow_buoyancy_options(C.Structure):
    """struct ow_buoyancy_options (64 bytes); zeros = the defaults (the query's, 1025 kg/m^3, 9.81 m/s^2, water level 0, cold start)"""
    _fields_ = [("query", ow_query_options), ("density", C.c_float), ("gravity", C.c_float), ("water_level", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class ow_buoyancy_point(C.Structure):
    """struct ow_buoyancy_point (64 bytes): one hull point's evaluation, also the warm start's state"""
    _fields_ = [("world", C.c_float * 3), ("height", C.c_float), ("depth", C.c_float), ("submerged", C.c_float), ("force", C.c_float * 3),
                ("p", C.c_float * 2), ("residual", C.c_float), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("converged", C.c_int32),
                ("body", C.c_int32)]


class ow_buoyancy_result(C.Structure):
    """struct ow_buoyancy_result (64 bytes): one body's force, torque about its origin, submerged volume and centre of buoyancy"""
    _fields_ = [("force", C.c_float * 3), ("torque", C.c_float * 3), ("submerged_volume", C.c_float), ("center_of_buoyancy", C.c_float * 3),
                ("wetted_points", C.c_int32), ("unconverged_points", C.c_int32), ("invalid_points", C.c_int32), ("max_residual", C.c_float),
                ("reserved", C.c_uint32 * 2)]


class ow_rigid_body(C.Structure):
    """struct ow_rigid_body (208 bytes): the FP64 state of a floating body (ow_bodies_create / ow_bodies_get_state / ow_bodies_set_state)"""
    _fields_ = [("position", C.c_double * 3), ("orientation", C.c_double * 4), ("linear_velocity", C.c_double * 3),
                ("angular_velocity", C.c_double * 3), ("mass", C.c_double), ("inverse_inertia", C.c_double * 3),
                ("applied_force", C.c_double * 3), ("applied_torque", C.c_double * 3), ("linear_drag", C.c_float), ("quadratic_drag", C.c_float),
                ("point_offset", C.c_int32), ("point_count", C.c_int32), ("reserved", C.c_uint32 * 2)]


class ow_bodies_options(C.Structure):
    """struct ow_bodies_options (80 bytes); zeros = the defaults of ow_buoyancy_options"""
    _fields_ = [("buoyancy", ow_buoyancy_options), ("reserved", C.c_uint32 * 4)]


class ow_ray(C.Structure):
    """struct ow_ray (32 bytes)"""
    _fields_ = [("origin", C.c_float * 3), ("max_distance", C.c_float), ("direction", C.c_float * 3), ("reserved", C.c_uint32)]


class ow_raycast_options(C.Structure):
    """struct ow_raycast_options (64 bytes); zeros = the defaults (the query's, water level 0, 0.25 m spacing, 1e-3 m, 4096 samples)"""
    _fields_ = [("query", ow_query_options), ("water_level", C.c_float), ("sample_spacing", C.c_float), ("tolerance", C.c_float),
                ("max_samples", C.c_int32), ("reserved", C.c_uint32 * 4)]


class ow_raycast_hit(C.Structure):
    """struct ow_raycast_hit (192 bytes): where a ray meets the water, the slab it searched, and the query record at the hit"""
    _fields_ = [("t", C.c_float), ("position", C.c_float * 3), ("residual", C.c_float), ("status", C.c_int32), ("samples", C.c_int32),
                ("rounds", C.c_int32), ("slab_half_height", C.c_float), ("t_enter", C.c_float), ("t_exit", C.c_float),
                ("reserved", C.c_uint32 * 5), ("query", ow_surface_query)]


class ow_camera(C.Structure):
    """struct ow_camera (80 bytes): position, Godot Transform3D basis rows (looking down -Z, +Y up), vertical fov in degrees, image size"""
    _fields_ = [("position", C.c_float * 3), ("max_distance", C.c_float), ("basis", C.c_float * 9), ("fov_y_degrees", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_uint32 * 4)]


class ow_render_options(C.Structure):
    """struct ow_render_options (192 bytes); a NULL pointer = ow_render_options_default's values, a given record is taken field by field"""
    _fields_ = [("raycast", ow_raycast_options), ("water_color", C.c_float * 3), ("roughness", C.c_float), ("foam_color", C.c_float * 3),
                ("normal_strength", C.c_float), ("light_direction", C.c_float * 3), ("flags", C.c_uint32), ("light_color", C.c_float * 3),
                ("ambient_color", C.c_float * 3), ("sky_color", C.c_float * 3), ("reserved", C.c_uint32 * 11)]


class ow_mesh_options(C.Structure):
    """struct ow_mesh_options (128 bytes); a NULL pointer = ow_mesh_options_default's values"""
    _fields_ = [("query_flags", C.c_uint32), ("falloff_center_xz", C.c_float * 2), ("near", C.c_float), ("water_color", C.c_float * 3),
                ("roughness", C.c_float), ("foam_color", C.c_float * 3), ("normal_strength", C.c_float), ("light_direction", C.c_float * 3),
                ("flags", C.c_uint32), ("light_color", C.c_float * 3), ("ambient_color", C.c_float * 3), ("sky_color", C.c_float * 3),
                ("lane_box", C.c_int32), ("reserved", C.c_uint32 * 6)]


class ow_spray_options(C.Structure):
    """struct ow_spray_options (128 bytes)"""
    _fields_ = [("amount", C.c_uint32), ("num_particles", C.c_uint32), ("emitter_lifetime", C.c_float), ("lifetime", C.c_float),
                ("lifetime_randomness", C.c_float), ("particle_scale", C.c_float * 3), ("random_seed", C.c_uint32), ("reserved0", C.c_uint32),
                ("emission_transform", C.c_float * 12), ("start_time", C.c_double), ("reserved", C.c_uint32 * 8)]


class ow_spray_instance(C.Structure):
    """struct ow_spray_instance (64 bytes): a particle's transform rows and custom data"""
    _fields_ = [("transform", C.c_float * 12), ("custom", C.c_float * 4)]


class ow_spray_particle(C.Structure):
    """struct ow_spray_particle (48 bytes): a particle's state"""
    _fields_ = [("start_pos", C.c_float * 3), ("start_time", C.c_float), ("particle_scale", C.c_float * 3), ("particle_lifetime", C.c_float),
                ("custom_z", C.c_float), ("scale_factor", C.c_float), ("flags", C.c_uint32), ("number", C.c_uint32)]


class ow_billboard_material_options(C.Structure):
    """struct ow_billboard_material_options (64 bytes): sea_spray.gdshader's uniforms and the textures' sRGB flags"""
    _fields_ = [("foam_color", C.c_float * 3), ("max_alpha", C.c_float), ("albedo_srgb", C.c_uint32), ("dissolve_srgb", C.c_uint32),
                ("reserved", C.c_uint32 * 10)]


class ow_billboard_draw_options(C.Structure):
    """struct ow_billboard_draw_options (64 bytes); a NULL pointer = near 0.05, a black background"""
    _fields_ = [("near", C.c_float), ("background_color", C.c_float * 3), ("bin_side", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 10)]


class ow_solid_options(C.Structure):
    """struct ow_solid_options (128 bytes); a NULL pointer = ow_solid_options_default's values"""
    _fields_ = [("near", C.c_float), ("color", C.c_float * 3), ("light_direction", C.c_float * 3), ("flags", C.c_uint32),
                ("light_color", C.c_float * 3), ("ambient_color", C.c_float * 3), ("background_color", C.c_float * 3), ("lane_box", C.c_int32),
                ("reserved", C.c_uint32 * 14)]


class ow_solid_cast_options(C.Structure):
    """struct ow_solid_cast_options (32 bytes); a NULL pointer = zeros: one-sided, culled by bounding spheres"""
    _fields_ = [("flags", C.c_uint32), ("cull", C.c_int32), ("reserved", C.c_uint32 * 6)]


class ow_solid_hit(C.Structure):
    """struct ow_solid_hit (64 bytes): where a ray meets the solids"""
    _fields_ = [("t", C.c_float), ("position", C.c_float * 3), ("normal", C.c_float * 3), ("status", C.c_int32), ("instance", C.c_int32),
                ("triangle", C.c_int32), ("barycentric", C.c_float * 2), ("reserved", C.c_uint32 * 4)]


class ow_sky_options(C.Structure):
    """struct ow_sky_options (32 bytes); a NULL pointer = srgb 1, energy 1"""
    _fields_ = [("srgb", C.c_uint32), ("energy", C.c_float), ("reserved", C.c_uint32 * 6)]


class ow_environment_options(C.Structure):
    """struct ow_environment_options (128 bytes); a NULL pointer = ow_environment_options_default's values (the reference scene's fog)"""
    _fields_ = [("fog_mode", C.c_int32), ("density", C.c_float), ("depth_begin", C.c_float), ("depth_end", C.c_float), ("depth_curve", C.c_float),
                ("aerial_perspective", C.c_float), ("sun_scatter", C.c_float), ("flags", C.c_uint32), ("light_color", C.c_float * 3),
                ("sun_color", C.c_float * 3), ("sun_direction", C.c_float * 3), ("sky_color", C.c_float * 3), ("reserved", C.c_uint32 * 12)]


class ow_present_options(C.Structure):
    """struct ow_present_options (64 bytes); a NULL pointer = ow_present_options_default's values (filmic, sRGB, the scene's adjustments)"""
    _fields_ = [("downsample", C.c_int32), ("tonemap", C.c_int32), ("exposure", C.c_float), ("white", C.c_float), ("srgb", C.c_uint32),
                ("brightness", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class ow_radiance_options(C.Structure):
    """struct ow_radiance_options (32 bytes); a NULL pointer = levels 6, samples 64, base_width 1024"""
    _fields_ = [("levels", C.c_int32), ("samples", C.c_int32), ("base_width", C.c_int32), ("reserved", C.c_uint32 * 5)]


class ow_radiance_light_options(C.Structure):
    """struct ow_radiance_light_options (64 bytes); a NULL pointer = ambient_energy 1, reflection_energy 1, specular 0.5"""
    _fields_ = [("ambient_energy", C.c_float), ("reflection_energy", C.c_float), ("specular", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 12)]


class ow_shadow_frame(C.Structure):
    """struct ow_shadow_frame (64 bytes): the light's orthographic box (ow_shadow_frame_default: the scene's sun over 100 m about the origin)"""
    _fields_ = [("light_direction", C.c_float * 3), ("half_extent", C.c_float), ("center", C.c_float * 3), ("depth_range", C.c_float),
                ("flags", C.c_uint32), ("lane_box", C.c_int32), ("reserved", C.c_uint32 * 6)]


class ow_shadow_options(C.Structure):
    """struct ow_shadow_options (64 bytes); a NULL pointer = bias 0, normal_bias 6.464, opacity 0.8, 5 taps, water does not receive"""
    _fields_ = [("bias", C.c_float), ("normal_bias", C.c_float), ("opacity", C.c_float), ("filter_taps", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 11)]


class ow_mist_options(C.Structure):
    """struct ow_mist_options (128 bytes); a NULL pointer = ow_mist_options_init's values (the reference scene's sea mist)"""
    _fields_ = [("extinction", C.c_float), ("height_falloff", C.c_float), ("base_height", C.c_float), ("length", C.c_float), ("anisotropy", C.c_float),
                ("sky_affect", C.c_float), ("slices", C.c_int32), ("flags", C.c_uint32), ("shadow_bias", C.c_float), ("albedo", C.c_float * 3),
                ("sun_color", C.c_float * 3), ("sun_direction", C.c_float * 3), ("ambient_color", C.c_float * 3), ("reserved", C.c_uint32 * 11)]


class ow_mirror_options(C.Structure):
    """struct ow_mirror_options (128 bytes); a NULL pointer = ow_mirror_options_init's values (the sky pass's and the solid draw's defaults)"""
    _fields_ = [("ambient_energy", C.c_float), ("reflection_energy", C.c_float), ("specular", C.c_float), ("body_color", C.c_float * 3),
                ("light_direction", C.c_float * 3), ("light_color", C.c_float * 3), ("ambient_color", C.c_float * 3), ("max_distance", C.c_float),
                ("fade_begin", C.c_float), ("opacity", C.c_float), ("flags", C.c_uint32), ("cull", C.c_int32), ("reserved", C.c_uint32 * 12)]


class ow_mesh_vertex(C.Structure):
    """struct ow_mesh_vertex (48 bytes): the vertex stage's record of a mesh draw"""
    _fields_ = [("position", C.c_float * 3), ("wave_height", C.c_float), ("uv", C.c_float * 2), ("distance_factor", C.c_float),
                ("reserved", C.c_uint32), ("view_position", C.c_float * 3), ("flags", C.c_uint32)]


class ow_render_pixel(C.Structure):
    """struct ow_render_pixel (128 bytes): the hit, the shader's inputs at it, fragment()'s and light()'s outputs and the composite"""
    _fields_ = [("t", C.c_float), ("status", C.c_int32), ("position", C.c_float * 3), ("p", C.c_float * 2), ("wave_height", C.c_float),
                ("gradient_fragment", C.c_float * 2), ("foam_fragment", C.c_float), ("dist", C.c_float), ("foam_factor", C.c_float),
                ("albedo", C.c_float * 3), ("normal", C.c_float * 3), ("fresnel", C.c_float), ("roughness", C.c_float),
                ("diffuse", C.c_float * 3), ("specular", C.c_float), ("color", C.c_float * 3), ("reserved", C.c_uint32 * 4)]


# every symbol include/ocean_waves.h declares: (restype, argtypes)
_P = C.POINTER
SIGNATURES = {
    "ow_create": (C.c_int, [_P(ow_config), _P(C.c_void_p)]),
    "ow_destroy": (None, [C.c_void_p]),
    "ow_cascade_params_default": (None, [_P(ow_cascade_params)]),
    "ow_update": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32]),
    "ow_set_cascade_params": (C.c_int, [C.c_void_p, C.c_int32, _P(ow_cascade_params)]),
    "ow_get_cascade_params": (C.c_int, [C.c_void_p, C.c_int32, _P(ow_cascade_params)]),
    "ow_debug_inject_fault": (C.c_int, [C.c_void_p, C.c_uint32]),
    "ow_debug_set_spectrum": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ow_get_push_constants": (C.c_int, [C.c_void_p, C.c_int32, _P(ow_push_constants)]),
    "ow_process": (C.c_int, [C.c_void_p]),
    "ow_update_all": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32]),
    "ow_run": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32, C.c_int32]),
    "ow_lookahead_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_spectrum_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_chain_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "ow_cascades_remaining": (C.c_int32, [C.c_void_p]),
    "ow_last_kernel_family": (C.c_int32, [C.c_void_p]),
    "ow_last_batch_cascades": (C.c_int32, [C.c_void_p]),
    "ow_tick_group_depth": (C.c_int32, [C.c_void_p]),
    "ow_sync": (C.c_int, [C.c_void_p]),
    "ow_get_device_ptrs": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_size_t)]),
    "ow_get_maps": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ow_set_normal_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_readback_begin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "ow_readback_wait": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p), _P(C.c_void_p)]),
    "ow_sample_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_query_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_query_options), C.c_void_p]),
    "ow_query_surface_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_query_options), C.c_void_p]),
    "ow_buoyancy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_buoyancy_options),
                              C.c_void_p, C.c_void_p]),
    "ow_buoyancy_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_buoyancy_options),
                                    C.c_void_p, C.c_void_p]),
    "ow_bodies_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "ow_bodies_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_bodies_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(ow_bodies_options), C.c_int32, C.c_double]),
    "ow_bodies_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ow_bodies_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ow_bodies_get_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ow_bodies_get_device_ptrs": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p)]),
    "ow_bodies_stats": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_sync_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "ow_raycast_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_raycast_options), C.c_void_p]),
    "ow_raycast_surface_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_raycast_options), C.c_void_p]),
    "ow_update_velocity": (C.c_int, [C.c_void_p, C.c_uint32]),
    "ow_get_velocity_ptrs": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "ow_get_velocity_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_velocity_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_query_velocity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_query_options), C.c_void_p]),
    "ow_query_velocity_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_query_options), C.c_void_p]),
    "ow_render_options_default": (None, [_P(ow_render_options)]),
    "ow_render_view": (C.c_int, [C.c_void_p, _P(ow_camera), C.c_void_p, C.c_int32, _P(ow_render_options), C.c_void_p, C.c_void_p]),
    "ow_render_view_async": (C.c_int, [C.c_void_p, _P(ow_camera), C.c_void_p, C.c_int32, _P(ow_render_options), C.c_void_p, C.c_void_p]),
    "ow_mesh_options_default": (None, [_P(ow_mesh_options)]),
    "ow_mesh_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "ow_mesh_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_mesh_displace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(ow_mesh_options), _P(ow_camera), C.c_void_p]),
    "ow_mesh_get_device_ptrs": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "ow_mesh_draw": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), C.c_void_p, C.c_void_p, C.c_int32, _P(ow_mesh_options), C.c_void_p, C.c_void_p]),
    "ow_mesh_draw_async": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), C.c_void_p, C.c_void_p, C.c_int32, _P(ow_mesh_options), C.c_void_p,
                                     C.c_void_p]),
    "ow_mesh_stats": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_spray_options_default": (None, [_P(ow_spray_options)]),
    "ow_spray_create": (C.c_int, [C.c_void_p, _P(ow_spray_options), _P(C.c_void_p)]),
    "ow_spray_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_spray_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int32]),
    "ow_spray_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_uint32)]),
    "ow_spray_get_device_ptrs": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p)]),
    "ow_spray_stats": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_double), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_billboard_material_options_default": (None, [_P(ow_billboard_material_options)]),
    "ow_billboard_material_create": (C.c_int, [C.c_void_p, _P(ow_billboard_material_options), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                               C.c_int32, _P(C.c_void_p)]),
    "ow_billboard_material_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_billboard_draw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_billboard_draw_options), C.c_void_p, C.c_void_p]),
    "ow_billboard_draw_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_billboard_draw_options), C.c_void_p, C.c_void_p]),
    "ow_billboard_draw_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, _P(ow_camera), _P(ow_billboard_draw_options),
                                              C.c_void_p, C.c_void_p]),
    "ow_billboard_draw_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_solid_options_default": (None, [_P(ow_solid_options)]),
    "ow_solid_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "ow_solid_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_solid_draw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(ow_camera), _P(ow_solid_options), C.c_void_p, C.c_void_p]),
    "ow_solid_draw_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(ow_camera), _P(ow_solid_options), C.c_void_p,
                                      C.c_void_p]),
    "ow_solid_draw_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(ow_camera), _P(ow_solid_options), C.c_void_p, C.c_void_p]),
    "ow_solid_draw_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_cast_bodies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, _P(ow_solid_cast_options),
                                    C.c_void_p]),
    "ow_cast_bodies_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                          _P(ow_solid_cast_options), C.c_void_p]),
    "ow_cast_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, _P(ow_solid_cast_options),
                                              C.c_void_p]),
    "ow_cast_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_sky_options_default": (None, [_P(ow_sky_options)]),
    "ow_environment_options_default": (None, [_P(ow_environment_options)]),
    "ow_present_options_default": (None, [_P(ow_present_options)]),
    "ow_sky_create": (C.c_int, [C.c_void_p, _P(ow_sky_options), C.c_void_p, C.c_int32, C.c_int32, _P(C.c_void_p)]),
    "ow_sky_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_environment_apply": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_environment_options), C.c_void_p]),
    "ow_environment_apply_async": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_environment_options), C.c_void_p]),
    "ow_present": (C.c_int, [C.c_void_p, _P(ow_camera), _P(ow_present_options), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ow_present_async": (C.c_int, [C.c_void_p, _P(ow_camera), _P(ow_present_options), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ow_radiance_options_default": (None, [_P(ow_radiance_options)]),
    "ow_radiance_light_options_default": (None, [_P(ow_radiance_light_options)]),
    "ow_radiance_create": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_radiance_options), _P(C.c_void_p)]),
    "ow_radiance_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_radiance_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ow_radiance_light_apply": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_radiance_light_options), C.c_void_p]),
    "ow_radiance_light_apply_async": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_radiance_light_options), C.c_void_p]),
    "ow_shadow_frame_default": (None, [_P(ow_shadow_frame)]),
    "ow_shadow_options_default": (None, [_P(ow_shadow_options)]),
    "ow_shadow_map_create": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "ow_shadow_map_destroy": (None, [C.c_void_p, C.c_void_p]),
    "ow_shadow_map_begin": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_shadow_frame)]),
    "ow_shadow_map_cast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "ow_shadow_map_cast_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "ow_shadow_map_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ow_shadow_apply": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_shadow_options), C.c_void_p, C.c_void_p]),
    "ow_shadow_apply_async": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_shadow_options), C.c_void_p, C.c_void_p]),
    "ow_shadow_stats": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_mist_options_init": (None, [_P(ow_mist_options)]),
    "ow_mist_apply": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_mist_options), C.c_void_p, C.c_void_p]),
    "ow_mist_apply_async": (C.c_int, [C.c_void_p, C.c_void_p, _P(ow_camera), _P(ow_mist_options), C.c_void_p, C.c_void_p]),
    "ow_mist_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_mirror_options_init": (None, [_P(ow_mirror_options)]),
    "ow_mirror_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(ow_camera), _P(ow_mirror_options), C.c_void_p,
                                  C.c_void_p]),
    "ow_mirror_apply_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(ow_camera), _P(ow_mirror_options),
                                        C.c_void_p, C.c_void_p]),
    "ow_mirror_apply_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(ow_camera), _P(ow_mirror_options), C.c_void_p,
                                            C.c_void_p]),
    "ow_mirror_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "ow_get_maps_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_get_spectrum": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ow_get_intermediate": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_jonswap_alpha": (C.c_double, [C.c_double, C.c_double]),
    "ow_jonswap_peak_angular_frequency": (C.c_double, [C.c_double, C.c_double]),
    "ow_timing_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "ow_timing_read": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float), _P(C.c_int32), C.c_int32]),
    "ow_timing_read_launches": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_int32), C.c_int32]),
    "ow_probe_kernel_times": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_float), _P(C.c_float), _P(C.c_int32)]),
    "ow_group_create": (C.c_int, [_P(ow_group_config), _P(C.c_void_p)]),
    "ow_group_destroy": (None, [C.c_void_p]),
    "ow_group_num_cascades": (C.c_int32, [C.c_void_p]),
    "ow_group_context": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "ow_group_update": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32]),
    "ow_group_process": (C.c_int, [C.c_void_p]),
    "ow_group_update_all": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32]),
    "ow_group_run": (C.c_int, [C.c_void_p, C.c_double, _P(ow_cascade_params), C.c_int32, C.c_int32]),
    "ow_group_cascades_remaining": (C.c_int32, [C.c_void_p]),
    "ow_group_sync": (C.c_int, [C.c_void_p]),
    "ow_group_gather_begin": (C.c_int, [C.c_void_p]),
    "ow_group_gather_wait": (C.c_int, [C.c_void_p]),
    "ow_group_gather_stats": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_size_t)]),
    "ow_group_link_info": (C.c_int, [C.c_void_p, C.c_int32, _P(ow_group_link)]),
    "ow_query_link": (C.c_int, [C.c_int32, C.c_int32, _P(ow_group_link)]),
    "ow_group_get_device_ptrs": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_size_t)]),
    "ow_group_get_maps": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ow_group_sample_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ow_group_query_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_query_options), C.c_void_p]),
    "ow_group_buoyancy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_buoyancy_options),
                                    C.c_void_p, C.c_void_p]),
    "ow_group_raycast_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(ow_raycast_options), C.c_void_p]),
    "ow_export_maps": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_size_t)]),
    "ow_import_buffer": (C.c_int, [C.c_int32, C.c_int32, C.c_size_t, C.c_size_t, _P(C.c_void_p), _P(C.c_void_p)]),
    "ow_release_buffer": (None, [C.c_void_p]),
    "ow_last_error": (C.c_char_p, []),
    "ow_abi_version": (C.c_int32, []),
}

_lib = None


def load():
    """Load libocean_waves.so (built in-tree by godotoceanwaves_amd.build).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OceanWavesError(-1, f"{LIB_PATH} is missing: run `python -m godotoceanwaves_amd.build` "
                                  "(hipcc, gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != OW_OK:
        raise OceanWavesError(status, load().ow_last_error().decode("utf-8", "replace"))
