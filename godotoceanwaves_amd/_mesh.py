"""A displaced water mesh drawn for a camera, on the device (csrc/ow_mesh_host.hip, include/ocean_waves.h ow_mesh_*)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _camera_xz, _create_shape, _data, _Mesh, _ref, _scales, _stats, Shared
from ._points import PointsCalls


class MeshCalls(Shared):
    _MESH_OWN = PointsCalls._RENDER_OWN + ("near", "cull_back", "lane_box", "falloff", "falloff_center")

    @staticmethod
    def clipmap_origin(camera_position, tile_size):
        """main.gd:34-37: where the water mesh is put for a camera -- ceil(camera.xz / tile) * tile, y = 0 -- as float32 (x, 0, z)"""
        xz = np.array([camera_position[0], camera_position[2]], np.float32)   # Vector3 is FP32
        t = np.float32(tile_size)
        out = np.ceil(xz / t) * t
        return np.array([out[0], 0.0, out[1]], np.float32)

    @classmethod
    def mesh_options(cls, options=None, camera=None):
        """None, an _lib.ow_mesh_options, or a dict -> ow_mesh_options, or None for the defaults.  The dict starts from
        ow_mesh_options_default's values and may set the shading keys of render_options, near, cull_back, lane_box and falloff_center;
        "falloff": True turns the shader's distance falloff on around the camera's x and z."""
        o = cls._options(_lib.ow_mesh_options, _lib.load().ow_mesh_options_default, cls._MESH_OWN, options, "mesh")
        if o is options:
            return o
        center = options.get("falloff_center")
        if options.get("falloff") and center is None:
            center = _camera_xz(camera)
        if center is not None:
            o.query_flags = _lib.OW_QUERY_DISTANCE_FALLOFF
            o.falloff_center_xz[:] = [float(v) for v in center]
        if options.get("cull_back"):
            o.flags |= _lib.OW_MESH_CULL_BACK
        return o

    def mesh_create(self, vertices, triangles):
        """A device-resident mesh from [V][3] local positions and [T][3] vertex indices; returns a _Mesh (mesh_destroy() it before free())"""
        return _Mesh(*_create_shape(self._lib.ow_mesh_create, self.context, vertices, triangles))

    def mesh_destroy(self, mesh):
        self._destroy(mesh, self._lib.ow_mesh_destroy)

    def mesh_displace(self, mesh, origin, map_scales, options=None, camera=None):
        """The vertex stage alone: MESH_VERTEX records of every vertex (view_position only with a camera); synchronises"""
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        out = np.zeros(mesh.num_vertices, self.MESH_VERTEX)
        _lib.check(self._lib.ow_mesh_displace(self.context, mesh.handle, org.ctypes.data, sc.ctypes.data, len(sc), _ref(o),
                                              _ref(camera), out.ctypes.data))
        return out

    def mesh_device_ptrs(self, mesh):
        """device addresses of the mesh's resident MESH_VERTEX records and of the context's visibility words (None before the first draw)"""
        v, w = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.ow_mesh_get_device_ptrs(self.context, mesh.handle, C.byref(v), C.byref(w)))
        return v.value, w.value

    def mesh_draw(self, mesh, camera, origin, map_scales, options=None, pixels=True):
        """The mesh as an ow_camera sees it: ((H, W, 4) uint8 RGBA, (H, W) RENDER_PIXEL records or None with pixels=False), rows from the
        top; a record's reserved[0] is the drawn triangle's index + 1."""
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        rgba, rec = self._picture(camera, True if pixels else None, True)
        _lib.check(self._lib.ow_mesh_draw(self.context, mesh.handle, C.byref(camera), org.ctypes.data, sc.ctypes.data, len(sc),
                                          _ref(o), rgba.ctypes.data, _data(rec)))
        return rgba, rec

    def mesh_draw_async(self, mesh, camera, origin, map_scales, rgba_device, pixels_device=None, options=None):
        """The draw over DEVICE buffers, enqueued in the generator's stream order without synchronising (render_view_async's buffers)"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        _lib.check(self._lib.ow_mesh_draw_async(self.context, mesh.handle, C.byref(camera), org.ctypes.data, sc.ctypes.data, len(sc),
                                                _ref(o), _addr(rgba_device, True), _addr(pixels_device, True)))

    def mesh_stats(self, mesh):
        """dict of draws and, of the last draw (synchronising), the triangles skipped, culled, per_lane and cooperative"""
        return _stats(self._lib.ow_mesh_stats, (self.context, mesh.handle), ("draws", "skipped", "culled", "per_lane", "cooperative"))
