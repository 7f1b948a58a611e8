"""The point calls of the wrapper (csrc/ow_points_host.hip): samples, queries, the surface's velocity, buoyancy, ray casts and camera views of
the water.  point_calls() writes the four host calls that a generator and a device group both have once, over either handle.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _camera_xz, _check_device_size, _count, _data, _fill, _ref, _scales, Shared

_QUERY_OWN = ("max_iterations", "tolerance", "falloff_center")
_BUOYANCY_OWN = ("density", "gravity", "water_level", "warm_start", "water_velocity")
_RAYCAST_OWN = ("water_level", "sample_spacing", "tolerance", "max_samples", "query_tolerance")


def _split(options, own):
    """(the dict's items under the keys in `own`, the others)"""
    return {k: v for k, v in options.items() if k in own}, {k: v for k, v in options.items() if k not in own}


def point_calls(prefix, handle):
    """The class of the four host point calls over the entry points prefix + name, on the handle the attribute `handle` holds: "ow_" and the
    context for WaveGenerator, "ow_group_" and the group (the gathered arrays on its root device) for WaveGeneratorGroup."""
    W = PointsCalls

    class PointCalls:
        def sample_surface(self, world_xz, map_scales):
            """Evaluate the water vertex/fragment sums and the sea-spray spawn mask at world points [P][2] (x, z);
            map_scales [C][4] as built by Water.map_scales() (water.gd:105-109).  Returns a structured array."""
            xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
            sc = _scales(map_scales)
            out = np.zeros(len(xz), W.SURFACE_SAMPLE)
            _lib.check(getattr(self._lib, prefix + "sample_surface")(getattr(self, handle), xz.ctypes.data, len(xz), sc.ctypes.data, len(sc),
                                                                     out.ctypes.data))
            return out

        def query_surface(self, world_xz, map_scales, options=None):
            """Where the rendered water is above world points [P][2] (x, z): the undisplaced point p, the residual, convergence, the
            rendered height and normal, and the full sample_surface record at p.  Returns a structured array (SURFACE_QUERY)."""
            xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
            sc = _scales(map_scales)
            out = np.zeros(len(xz), W.SURFACE_QUERY)
            o = W.query_options(options)
            _lib.check(getattr(self._lib, prefix + "query_surface")(getattr(self, handle), xz.ctypes.data, len(xz), sc.ctypes.data, len(sc),
                                                                    _ref(o), out.ctypes.data))
            return out

        def buoyancy(self, bodies, hull, map_scales, options=None, points=None):
            """Force, torque, submerged volume and centre of buoyancy per body (BUOYANCY_RESULT records) for BUOYANCY_BODY records over
            HULL_POINT records, on the device.  points: None, or a BUOYANCY_POINT array of len(hull) that receives the per-point records
            (and holds the previous step's for the warm start, options {"warm_start": True})."""
            b = np.ascontiguousarray(bodies, W.BUOYANCY_BODY)
            h = np.ascontiguousarray(hull, W.HULL_POINT)
            sc = _scales(map_scales)
            if points is not None and (not isinstance(points, np.ndarray) or points.dtype != W.BUOYANCY_POINT or len(points) != len(h)
                                       or not points.flags.c_contiguous):
                raise ValueError(f"points must be a contiguous BUOYANCY_POINT array of {len(h)} records")
            out = np.zeros(len(b), W.BUOYANCY_RESULT)
            o = W.buoyancy_options(options)
            _lib.check(getattr(self._lib, prefix + "buoyancy")(getattr(self, handle), b.ctypes.data, len(b), h.ctypes.data, len(h), sc.ctypes.data,
                                                               len(sc), _ref(o), out.ctypes.data, _data(points)))
            return out

        def raycast_surface(self, rays, map_scales, options=None):
            """Where each RAY record first meets the rendered water: t, the position, the status bits (_lib.OW_RAY_*), the slab searched
            and the SURFACE_QUERY record at the hit.  Returns a structured array (RAYCAST_HIT)."""
            r = np.ascontiguousarray(rays, W.RAY)
            sc = _scales(map_scales)
            out = np.zeros(len(r), W.RAYCAST_HIT)
            o = W.raycast_options(options)
            _lib.check(getattr(self._lib, prefix + "raycast_surface")(getattr(self, handle), r.ctypes.data, len(r), sc.ctypes.data, len(sc),
                                                                      _ref(o), out.ctypes.data))
            return out

    return PointCalls


class PointsCalls(Shared):
    # ---- the water above a world point: p + f(p) D(p) = q solved on the device (include/ocean_waves.h ow_query_surface) ----
    @staticmethod
    def query_options(options=None):
        """None, an _lib.ow_query_options, or a dict of max_iterations / tolerance / falloff_center ((x, z): the camera position
        of water.gdshader:29's distance falloff) -> ow_query_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_query_options):
            return options
        o = Shared._options(_lib.ow_query_options, None, _QUERY_OWN, dict(sorted(options.items())), "query")   # unknown keys are named sorted
        if options.get("falloff_center") is not None:
            o.flags = _lib.OW_QUERY_DISTANCE_FALLOFF
            o.falloff_center_xz[0], o.falloff_center_xz[1] = (float(v) for v in options["falloff_center"])
        return o

    def query_surface_async(self, xz_device, map_scales, out_device, options=None, count=None):
        """The query over DEVICE buffers, enqueued in the generator's stream order without synchronising: xz_device holds 2 * count
        float32 (x, z pairs), out_device room for count 128-byte records.  Each is anything with a data_ptr() (a torch tensor) or an
        integer address; count defaults to xz_device.numel() // 2."""
        count = _count(count, xz_device, 2)
        _check_device_size(out_device, count, self.SURFACE_QUERY.itemsize)
        sc = _scales(map_scales)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_surface_async(self.context, _addr(xz_device), int(count), sc.ctypes.data, len(sc),
                                                    _ref(o), _addr(out_device)))

    # ---- buoyancy: per-body force and torque from hull points, on the device (include/ocean_waves.h ow_buoyancy) ----
    @classmethod
    def buoyancy_options(cls, options=None):
        """None, an _lib.ow_buoyancy_options, or a dict of density / gravity / water_level / warm_start (bool) / water_velocity (bool: drag
        relative to the moving surface) and the query_options keys -> ow_buoyancy_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_buoyancy_options):
            return options
        own, rest = _split(options, _BUOYANCY_OWN)
        q = cls.query_options(rest)                     # the other keys are the query's: "unknown query options"
        o = cls._options(_lib.ow_buoyancy_options, None, _BUOYANCY_OWN, own, "buoyancy")
        o.flags = (_lib.OW_BUOYANCY_WARM_START if own.get("warm_start") else 0) | (_lib.OW_BUOYANCY_WATER_VELOCITY if own.get("water_velocity") else 0)
        o.query = q
        return o

    @classmethod
    def box_hull(cls, size, divisions, body=0, center=(0.0, 0.0, 0.0)):
        """A box of size (x, y, z) metres centred at `center` (body space) voxelised into divisions (i, j, k) cells: one hull point per
        cell at its centre, volume = the cell's volume, half_height = half the cell's height.  Returns HULL_POINT records of `body`."""
        size = np.asarray(size, np.float64)
        div = np.asarray(divisions, np.int64)
        cell = size / div
        axes = [(np.arange(d) + 0.5) * c - s / 2 + o for d, c, s, o in zip(div, cell, size, center)]
        X, Y, Z = np.meshgrid(*axes, indexing="ij")
        out = np.zeros(X.size, cls.HULL_POINT)
        out["local"] = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
        out["volume"] = np.prod(cell)
        out["half_height"] = cell[1] / 2
        out["body"] = body
        return out

    def buoyancy_async(self, bodies_device, hull_device, map_scales, results_device, points_device, options=None, num_bodies=None,
                       num_points=None):
        """ow_buoyancy_async over DEVICE buffers (torch tensors or integer addresses), enqueued in the generator's stream order without
        synchronising.  The counts default to the tensors' byte sizes over the record sizes."""
        nb = _count(num_bodies, bodies_device, self.BUOYANCY_BODY, "num_bodies")
        npts = _count(num_points, hull_device, self.HULL_POINT, "num_points")
        _check_device_size(results_device, nb, self.BUOYANCY_RESULT.itemsize, "results_device")
        _check_device_size(points_device, npts, self.BUOYANCY_POINT.itemsize, "points_device")
        sc = _scales(map_scales)
        o = self.buoyancy_options(options)
        _lib.check(self._lib.ow_buoyancy_async(self.context, _addr(bodies_device), nb, _addr(hull_device), npts, sc.ctypes.data, len(sc),
                                               _ref(o), _addr(results_device), _addr(points_device)))

    # ---- ray casts against the rendered water, on the device (include/ocean_waves.h ow_raycast_surface) ----
    @classmethod
    def rays(cls, origins, directions, max_distance):
        """RAY records from origins [R][3], directions [R][3] (any non-zero length) and max_distance (a scalar or [R]).  Godot's
        intersect_ray(from, to): origin = from, direction = to - from, max_distance = |to - from|."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        out = np.zeros(len(o), cls.RAY)
        out["origin"] = o
        out["direction"] = np.asarray(directions, np.float32).reshape(-1, 3)
        out["max_distance"] = max_distance
        return out

    @classmethod
    def raycast_options(cls, options=None):
        """None, an _lib.ow_raycast_options, or a dict of water_level / sample_spacing / tolerance / max_samples and the query_options
        keys (query_tolerance for the query's own tolerance) -> ow_raycast_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_raycast_options):
            return options
        own, q = _split(options, _RAYCAST_OWN)
        if "query_tolerance" in own:
            q["tolerance"] = own["query_tolerance"]
        qo = cls.query_options(q) if q else None        # a query is built only where a key asks for one
        o = cls._options(_lib.ow_raycast_options, None, _RAYCAST_OWN, own, "raycast")
        if qo is not None:
            o.query = qo
        return o

    def raycast_surface_async(self, rays_device, map_scales, out_device, options=None, count=None):
        """The ray casts over DEVICE buffers, enqueued in the generator's stream order without synchronising: rays_device holds count
        32-byte RAY records, out_device room for count 192-byte records.  Each is anything with a data_ptr() (a torch tensor) or an
        integer address; count defaults to the byte size of rays_device over 32."""
        count = _count(count, rays_device, self.RAY)
        _check_device_size(out_device, count, self.RAYCAST_HIT.itemsize)
        sc = _scales(map_scales)
        o = self.raycast_options(options)
        _lib.check(self._lib.ow_raycast_surface_async(self.context, _addr(rays_device), int(count), sc.ctypes.data, len(sc),
                                                      _ref(o), _addr(out_device)))

    # ---- the water's velocity: V = dD/dt per layer, and the surface's velocity above world points (include/ocean_waves.h ow_update_velocity) ----
    def update_velocity(self, cascades=None):
        """enqueue the refresh of the stale velocity layers among `cascades` (indices; None = all), without synchronising"""
        mask = (1 << self.num_cascades) - 1 if cascades is None else sum(1 << int(i) for i in cascades)
        _lib.check(self._lib.ow_update_velocity(self.context, mask))

    def velocity_ptrs(self):
        """(device address of the velocity array, layer stride in bytes), every computed layer refreshed first"""
        p, st = C.c_void_p(), C.c_size_t()
        _lib.check(self._lib.ow_get_velocity_ptrs(self.context, C.byref(p), C.byref(st)))
        return p.value, st.value

    def velocity_map(self, cascade):
        """layer `cascade` of the velocity array as FP16 [N][N][4]: (dD_x/dt, dD_y/dt, dD_z/dt, 0) in m/s, before displacement_scale"""
        n = self.map_size
        out = np.empty((n, n, 4), np.float16)
        _lib.check(self._lib.ow_get_velocity_map(self.context, int(cascade), out.ctypes.data))
        return out

    def velocity_stats(self):
        """(computed, skipped): velocity layers computed, and layers asked for that were current already"""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_velocity_stats(self.context, C.byref(a), C.byref(b)))
        return a.value, b.value

    def query_velocity(self, world_xz, map_scales, options=None):
        """The velocity of the rendered surface above world points [P][2] (x, z), with ow_query_surface's height, p and convergence.
        Returns a structured array (SURFACE_VELOCITY)."""
        xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
        sc = _scales(map_scales)
        out = np.zeros(len(xz), self.SURFACE_VELOCITY)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_velocity(self.context, xz.ctypes.data, len(xz), sc.ctypes.data, len(sc),
                                               _ref(o), out.ctypes.data))
        return out

    def query_velocity_async(self, xz_device, map_scales, out_device, options=None, count=None):
        """query_velocity over DEVICE buffers, as query_surface_async (out_device: room for count 32-byte records)"""
        count = _count(count, xz_device, 2)
        _check_device_size(out_device, count, self.SURFACE_VELOCITY.itemsize)
        sc = _scales(map_scales)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_velocity_async(self.context, _addr(xz_device), int(count), sc.ctypes.data, len(sc),
                                                     _ref(o), _addr(out_device)))

    # ---- camera views of the water, on the device (include/ocean_waves.h ow_render_view) ----
    _RENDER_OWN = ("water_color", "foam_color", "roughness", "normal_strength", "light_direction", "light_color", "ambient_color", "sky_color")

    @staticmethod
    def camera(position, basis, fov_y_degrees, width, height, max_distance):
        """an _lib.ow_camera from a position, Godot Transform3D basis rows (9 values or 3 x 3; the camera looks down its -Z, +Y is up),
        the vertical field of view in degrees, the image size and the length of each pixel's ray"""
        cam = _lib.ow_camera(max_distance=float(max_distance), fov_y_degrees=float(fov_y_degrees), width=int(width), height=int(height))
        cam.position[:] = [float(v) for v in position]
        cam.basis[:] = [float(v) for v in np.asarray(basis, np.float64).reshape(9)]
        return cam

    @classmethod
    def _set_material(cls, o, options):
        """the material and light keys of render_options (_RENDER_OWN) out of a dict that holds the ray cast's keys as well, into the struct"""
        _fill(o, _split(options, cls._RENDER_OWN)[0])

    @classmethod
    def render_options(cls, options=None, camera=None):
        """None, an _lib.ow_render_options, or a dict -> ow_render_options, or None for the defaults.  The dict starts from
        ow_render_options_default's values and may set water_color / foam_color / roughness / normal_strength / light_direction /
        light_color / ambient_color / sky_color and the raycast_options keys.  "falloff": True turns the shader's distance falloff on
        around the camera's x and z (falloff_center names another centre)."""
        if options is None or isinstance(options, _lib.ow_render_options):
            return options
        o = _lib.ow_render_options()
        _lib.load().ow_render_options_default(C.byref(o))
        ray = _split(options, cls._RENDER_OWN + ("falloff",))[1]      # the other keys are the ray cast's: "unknown query options"
        if options.get("falloff") and ray.get("falloff_center") is None:
            ray["falloff_center"] = _camera_xz(camera)
        if ray:
            o.raycast = cls.raycast_options(ray)
        cls._set_material(o, options)
        return o

    def render_view(self, camera, map_scales, options=None, pixels=True):
        """The view of an ow_camera (WaveGenerator.camera): ((H, W, 4) uint8 RGBA, (H, W) structured RENDER_PIXEL records, or None with
        pixels=False), rows from the top."""
        sc = _scales(map_scales)
        o = self.render_options(options, camera)
        rgba, rec = self._picture(camera, True if pixels else None, True)
        _lib.check(self._lib.ow_render_view(self.context, C.byref(camera), sc.ctypes.data, len(sc), _ref(o), rgba.ctypes.data, _data(rec)))
        return rgba, rec

    def render_view_async(self, camera, map_scales, rgba_device, pixels_device=None, options=None):
        """The view over DEVICE buffers, enqueued in the generator's stream order without synchronising: rgba_device holds H * W * 4 bytes,
        pixels_device H * W 128-byte records; each is anything with a data_ptr() (a torch tensor), an integer address, or None (not both)."""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        sc = _scales(map_scales)
        o = self.render_options(options, camera)
        _lib.check(self._lib.ow_render_view_async(self.context, C.byref(camera), sc.ctypes.data, len(sc), _ref(o),
                                                  _addr(rgba_device, True), _addr(pixels_device, True)))
