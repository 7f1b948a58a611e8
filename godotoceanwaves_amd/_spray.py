"""The sea-spray particle emitter and its billboards drawn into a camera view, on the device (csrc/ow_spray_host.hip, include/ocean_waves.h
ow_spray_*, ow_billboard_*)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _data, _ref, _scales, _Spray, _SprayMaterial, _stats, Shared


def _flat(n):
    """a spray option's array, given flat or nested, as n float32"""
    return lambda v: np.asarray(v, np.float32).reshape(n)


class SprayCalls(Shared):
    _SPRAY_OWN = ("amount", "num_particles", "emitter_lifetime", "lifetime", "lifetime_randomness", "particle_scale", "random_seed",
                  "emission_transform", "start_time")
    _SPRAY_MATERIAL_OWN = ("foam_color", "max_alpha", "albedo_srgb", "dissolve_srgb")
    _SPRAY_DRAW_OWN = ("near", "background_color", "bin_side")

    @classmethod
    def spray_options(cls, options=None):
        """None, an _lib.ow_spray_options, or a dict -> ow_spray_options.  The dict starts from ow_spray_options_default's values (the
        reference scene's emitter) and may set amount, num_particles, emitter_lifetime, lifetime, lifetime_randomness, particle_scale,
        random_seed, emission_transform (3 x 4) and start_time."""
        return cls._options(_lib.ow_spray_options, _lib.load().ow_spray_options_default, cls._SPRAY_OWN, options or {}, "spray",
                            {"particle_scale": _flat(3), "emission_transform": _flat(12)})

    def spray_create(self, options=None):
        """A device-resident emitter, every particle dormant; returns a _Spray (spray_destroy() it before free())"""
        o = self.spray_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_spray_create(self.context, C.byref(o), C.byref(out)))
        return _Spray(out, int(o.amount))

    def spray_destroy(self, spray):
        self._destroy(spray, self._lib.ow_spray_destroy)

    def spray_step(self, spray, delta, map_scales):
        """One frame of the emitter on the maps as they stand in the generator's stream order; enqueues and returns"""
        sc = _scales(map_scales)
        _lib.check(self._lib.ow_spray_step(self.context, spray.handle, float(delta), sc.ctypes.data, len(sc)))

    def spray_read(self, spray):
        """(SPRAY_INSTANCE[amount], SPRAY_PARTICLE[amount], draw list uint32[live_count]) as the last step left them; synchronises"""
        inst, part = np.zeros(spray.amount, self.SPRAY_INSTANCE), np.zeros(spray.amount, self.SPRAY_PARTICLE)
        draw, live = np.zeros(spray.amount, np.uint32), C.c_uint32()
        _lib.check(self._lib.ow_spray_read(self.context, spray.handle, inst.ctypes.data, part.ctypes.data, draw.ctypes.data, C.byref(live)))
        return inst, part, draw[:live.value].copy()

    def spray_live_count(self, spray):
        live = C.c_uint32()
        _lib.check(self._lib.ow_spray_read(self.context, spray.handle, None, None, None, C.byref(live)))
        return live.value

    def spray_device_ptrs(self, spray):
        """device addresses of the instances, the state records, the draw list and the live count"""
        v = [C.c_void_p() for _ in range(4)]
        _lib.check(self._lib.ow_spray_get_device_ptrs(self.context, spray.handle, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def spray_stats(self, spray):
        """dict of time, steps, restarts (the host's bookkeeping) and spawned, rejected (summed on the device; synchronises)"""
        return _stats(self._lib.ow_spray_stats, (self.context, spray.handle), ("time", "steps", "restarts", "spawned", "rejected"),
                      kinds={"time": C.c_double})

    # ---- the spray billboards drawn into a camera view (include/ocean_waves.h ow_billboard_*) ----
    @classmethod
    def spray_material_options(cls, options=None):
        """None, an _lib.ow_billboard_material_options, or a dict over ow_billboard_material_options_default's values (the reference scene's
        foam colour, max_alpha 0.666, both textures sRGB) that may set foam_color, max_alpha, albedo_srgb and dissolve_srgb"""
        return cls._options(_lib.ow_billboard_material_options, _lib.load().ow_billboard_material_options_default, cls._SPRAY_MATERIAL_OWN,
                            options or {}, "spray material")

    @classmethod
    def spray_draw_options(cls, options=None):
        """None, an _lib.ow_billboard_draw_options, or a dict of near, background_color and bin_side -> ow_billboard_draw_options or None"""
        return cls._options(_lib.ow_billboard_draw_options, None, cls._SPRAY_DRAW_OWN, options, "spray draw")

    def spray_material_create(self, albedo_rgba8, dissolve_rgba8, options=None):
        """A billboard material from two (H, W, 4) uint8 textures, uploaded once; returns a _SprayMaterial (spray_material_destroy() it
        before free())"""
        a, d = (np.ascontiguousarray(t, np.uint8) for t in (albedo_rgba8, dissolve_rgba8))
        for t in (a, d):
            if t.ndim != 3 or t.shape[2] != 4:
                raise ValueError("a texture is (height, width, 4) uint8")
        o = self.spray_material_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_billboard_material_create(self.context, C.byref(o), a.ctypes.data, a.shape[1], a.shape[0], d.ctypes.data, d.shape[1],
                                                          d.shape[0], C.byref(out)))
        return _SprayMaterial(out)

    def spray_material_destroy(self, material):
        self._destroy(material, self._lib.ow_billboard_material_destroy)

    def spray_draw(self, spray, material, camera, options=None, pixels=None, rgba=True):
        """The emitter's live particles blended over `pixels` ((H, W) RENDER_PIXEL records of mesh_draw or render_view; None: the options'
        background colour, no depth): ((H, W, 4) uint8 RGBA, the records rewritten or None); a record's reserved[1] counts the fragments
        blended, reserved[2] is the last one's particle index + 1.  Synchronises."""
        o = self.spray_draw_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_billboard_draw(self.context, spray.handle, material.handle, C.byref(camera), _ref(o), _data(rec), _data(img)))
        return img, rec

    def spray_draw_instances(self, material, instances, time, camera, options=None, pixels=None, rgba=True):
        """spray_draw over a host array of SPRAY_INSTANCE records, drawn in array order, with TIME = time"""
        inst = np.ascontiguousarray(instances, self.SPRAY_INSTANCE).reshape(-1)
        o = self.spray_draw_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_billboard_draw_instances(self.context, material.handle, inst.ctypes.data if len(inst) else None, len(inst), float(time),
                                                         C.byref(camera), _ref(o), _data(rec), _data(img)))
        return img, rec

    def spray_draw_async(self, spray, material, camera, rgba_device, pixels_device=None, options=None):
        """The draw over DEVICE buffers (mesh_draw_async's), enqueued in the generator's stream order without synchronising; the records are
        read and rewritten in place"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        o = self.spray_draw_options(options)
        _lib.check(self._lib.ow_billboard_draw_async(self.context, spray.handle, material.handle, C.byref(camera), _ref(o),
                                                     _addr(pixels_device, True), _addr(rgba_device, True)))

    def spray_draw_stats(self, counters=True):
        """dict of draws, the scratch bytes held and, with counters (synchronising), the billboards the last draw culled and drawn"""
        return _stats(self._lib.ow_billboard_draw_stats, (self.context,), ("draws", "culled", "drawn", "scratch_bytes"),
                      () if counters else ("culled", "drawn"))
