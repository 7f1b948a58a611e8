"""Solids drawn into a camera view and the floating bodies' sun shadows, on the device (csrc/ow_solid_host.hip, include/ocean_waves.h
ow_solid_*, ow_shadow_*)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _create_shape, _data, _handle, _ref, _rest, _Solid, _stats, ShadowMap, Shared


class SolidCalls(Shared):
    _SOLID_OWN = ("near", "color", "light_direction", "light_color", "ambient_color", "background_color", "two_sided", "lane_box")

    @classmethod
    def solid_options(cls, options=None):
        """None, an _lib.ow_solid_options, or a dict over ow_solid_options_default's values (the reference scene's sun and ambient, a brown
        albedo) that may set near, color, light_direction, light_color, ambient_color, background_color, two_sided and lane_box"""
        o = cls._options(_lib.ow_solid_options, _lib.load().ow_solid_options_default, cls._SOLID_OWN, options, "solid")
        if o is not options and options.get("two_sided"):
            o.flags |= _lib.OW_SOLID_TWO_SIDED
        return o

    def solid_create(self, vertices, triangles):
        """A device-resident shape from [V][3] local positions and [T][3] vertex indices (counter-clockwise seen from outside); returns a
        _Solid (solid_destroy() it before free())"""
        return _Solid(*_create_shape(self._lib.ow_solid_create, self.context, vertices, triangles))

    def solid_destroy(self, solid):
        self._destroy(solid, self._lib.ow_solid_destroy)

    def solid_draw(self, solid, bodies_set, camera, options=None, pixels=None, rgba=True, first=0, count=None):
        """The shape at the resident poses of bodies [first, first + count) of a body set, drawn over `pixels` ((H, W) RENDER_PIXEL records of
        mesh_draw or render_view; None: the options' background colour, no depth): ((H, W, 4) uint8 RGBA, the records rewritten or None).  A
        record a solid wins carries OW_RAY_SOLID, reserved[0] the triangle's index + 1 and reserved[3] the instance's index + 1.
        Synchronises."""
        o = self.solid_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_solid_draw(self.context, solid.handle, bodies_set.handle, int(first), int(_rest(bodies_set, first, count)),
                                           C.byref(camera), _ref(o), _data(rec), _data(img)))
        return img, rec

    def solid_draw_instances(self, solid, transforms, camera, options=None, pixels=None, rgba=True):
        """solid_draw over a host array of [count][12] transforms (basis rows, then the origin)"""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
        o = self.solid_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_solid_draw_instances(self.context, solid.handle, t.ctypes.data if len(t) else None, len(t), C.byref(camera), _ref(o),
                                                     _data(rec), _data(img)))
        return img, rec

    def solid_draw_async(self, solid, bodies_set, camera, rgba_device, pixels_device=None, options=None, first=0, count=None):
        """The draw over DEVICE buffers (mesh_draw_async's), enqueued in the generator's stream order without synchronising; the records are
        read and rewritten in place"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        o = self.solid_options(options)
        _lib.check(self._lib.ow_solid_draw_async(self.context, solid.handle, bodies_set.handle, int(first), int(_rest(bodies_set, first, count)),
                                                 C.byref(camera), _ref(o), _addr(pixels_device, True), _addr(rgba_device, True)))

    def solid_draw_stats(self, counters=True):
        """dict of draws, the scratch bytes held and, with counters (synchronising), the instances the last draw skipped and the triangles
        it culled and drew"""
        return _stats(self._lib.ow_solid_draw_stats, (self.context,), ("draws", "skipped_instances", "culled", "drawn", "scratch_bytes"),
                      () if counters else ("skipped_instances", "culled", "drawn"))

    # ---- the floating bodies' sun shadows (include/ocean_waves.h ow_shadow_*) ----
    _SHADOW_FRAME_OWN = ("light_direction", "half_extent", "center", "depth_range", "cast_both_sides", "lane_box")
    _SHADOW_OWN = ("bias", "normal_bias", "opacity", "filter_taps", "receive_water")

    @classmethod
    def shadow_frame(cls, frame=None):
        """an _lib.ow_shadow_frame, or None / a dict of light_direction, half_extent, center, depth_range, cast_both_sides and lane_box over
        ow_shadow_frame_default's values (the scene's sun, 100 m about the origin, 100 m either side along the light)"""
        frame = frame or {}      # None is the default's frame; a struct passes
        o = cls._options(_lib.ow_shadow_frame, _lib.load().ow_shadow_frame_default, cls._SHADOW_FRAME_OWN, frame, "shadow frame")
        if o is not frame and frame.get("cast_both_sides"):
            o.flags |= _lib.OW_SHADOW_CAST_BOTH_SIDES
        return o

    @classmethod
    def shadow_options(cls, options=None):
        """None, an _lib.ow_shadow_options, or a dict of bias, normal_bias, opacity, filter_taps and receive_water over
        ow_shadow_options_default's values (0, 6.464, 0.8, 5 taps, water does not receive)"""
        o = cls._options(_lib.ow_shadow_options, _lib.load().ow_shadow_options_default, cls._SHADOW_OWN, options, "shadow")
        if o is not options and options.get("receive_water"):
            o.flags |= _lib.OW_SHADOW_RECEIVE_WATER
        return o

    def shadow_map_create(self, size):
        """An empty size x size depth map from the sun, without a frame; returns a ShadowMap (shadow_map_destroy() it before free())"""
        out = C.c_void_p()
        _lib.check(self._lib.ow_shadow_map_create(self.context, int(size), C.byref(out)))
        return ShadowMap(out, int(size))

    def shadow_map_destroy(self, shadow_map):
        self._destroy(shadow_map, self._lib.ow_shadow_map_destroy)

    def shadow_map_begin(self, shadow_map, frame=None):
        """Sets the frame and clears the map and its counters, enqueued in the generator's stream order without synchronising"""
        _lib.check(self._lib.ow_shadow_map_begin(self.context, shadow_map.handle, C.byref(self.shadow_frame(frame))))

    def shadow_map_cast(self, shadow_map, solid, bodies_set, first=0, count=None):
        """Casts the shape at the resident poses of bodies [first, first + count) into the map, enqueued without synchronising"""
        _lib.check(self._lib.ow_shadow_map_cast(self.context, shadow_map.handle, solid.handle, bodies_set.handle, int(first),
                                                int(_rest(bodies_set, first, count))))

    def shadow_map_cast_instances(self, shadow_map, solid, transforms):
        """shadow_map_cast over a host array of [count][12] transforms (basis rows, then the origin).  Synchronises."""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
        _lib.check(self._lib.ow_shadow_map_cast_instances(self.context, shadow_map.handle, solid.handle, t.ctypes.data if len(t) else None, len(t)))

    def shadow_map_read(self, shadow_map):
        """(size, size) float32 depths in metres from the frame's near plane, FLT_MAX where nothing was cast.  Synchronises."""
        out = np.zeros((shadow_map.size, shadow_map.size), np.float32)
        _lib.check(self._lib.ow_shadow_map_read(self.context, shadow_map.handle, out.ctypes.data))
        return out

    def shadow_apply(self, shadow_map, camera, pixels, options=None, rgba=False):
        """The sun's share of `pixels` ((H, W) RENDER_PIXEL records of the draws) darkened by the map: (the (H, W, 4) uint8 RGBA image or
        None, the records with status, diffuse, specular and color rewritten (a copy)).  Call it after solid_draw and before
        sky_light_apply and environment_apply.  Synchronises."""
        o = self.shadow_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_shadow_apply(self.context, _handle(shadow_map), C.byref(camera), _ref(o), rec.ctypes.data, _data(img)))
        return img, rec

    def shadow_apply_async(self, shadow_map, camera, pixels_device, rgba_device=None, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        o = self.shadow_options(options)
        _lib.check(self._lib.ow_shadow_apply_async(self.context, _handle(shadow_map), C.byref(camera), _ref(o), _addr(pixels_device),
                                                   _addr(rgba_device, True)))

    def shadow_stats(self, shadow_map, counters=True):
        """dict of the casts since the map's last begin, the scratch bytes held and, with counters (synchronising), the instances skipped and
        the triangles culled and drawn"""
        return _stats(self._lib.ow_shadow_stats, (self.context, shadow_map.handle), ("casts", "skipped_instances", "culled", "drawn", "scratch_bytes"),
                      () if counters else ("skipped_instances", "culled", "drawn"))
