"""The finishing stage of a camera picture, on the device: sky, fog, tonemap, sRGB, and the sky's prefiltered light (csrc/ow_sky_host.hip,
include/ocean_waves.h ow_sky_*, ow_environment_apply, ow_present, ow_radiance_*)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _check_device_size, _data, _handle, _ref, Radiance, Shared, Sky


class SkyCalls(Shared):
    _SKY_OWN = ("srgb", "energy")
    _ENVIRONMENT_OWN = ("fog_mode", "density", "depth_begin", "depth_end", "depth_curve", "aerial_perspective", "sun_scatter", "light_color", "sun_color",
                        "sun_direction", "sky_color")
    _PRESENT_OWN = ("downsample", "tonemap", "exposure", "white", "srgb", "brightness", "contrast", "saturation")
    FOG_MODES = {"exponential": _lib.OW_FOG_EXPONENTIAL, "depth": _lib.OW_FOG_DEPTH}
    TONEMAPS = {"linear": _lib.OW_TONEMAP_LINEAR, "reinhard": _lib.OW_TONEMAP_REINHARD, "filmic": _lib.OW_TONEMAP_FILMIC}

    @classmethod
    def sky_options(cls, options=None):
        """None, an _lib.ow_sky_options, or a dict of srgb and energy over ow_sky_options_default's values"""
        return cls._options(_lib.ow_sky_options, _lib.load().ow_sky_options_default, cls._SKY_OWN, options, "sky")

    @classmethod
    def environment_options(cls, options=None):
        """None, an _lib.ow_environment_options, or a dict over ow_environment_options_default's values (the reference scene's depth fog) that may
        set fog_mode ("depth" / "exponential" or the number), density, depth_begin, depth_end, depth_curve, aerial_perspective, sun_scatter,
        light_color, sun_color, sun_direction and sky_color"""
        return cls._options(_lib.ow_environment_options, _lib.load().ow_environment_options_default, cls._ENVIRONMENT_OWN, options, "environment",
                            {"fog_mode": cls.FOG_MODES})

    @classmethod
    def present_options(cls, options=None):
        """None, an _lib.ow_present_options, or a dict over ow_present_options_default's values (filmic, sRGB, the scene's adjustments) that may
        set downsample, tonemap ("linear" / "reinhard" / "filmic" or the number), exposure, white, srgb, brightness, contrast and saturation"""
        return cls._options(_lib.ow_present_options, _lib.load().ow_present_options_default, cls._PRESENT_OWN, options, "present",
                            {"tonemap": cls.TONEMAPS})

    def sky_create(self, panorama_rgba8, options=None):
        """A panorama from an (H, W, 4) uint8 equirectangular image, rows from the top, uploaded once; returns a Sky (sky_destroy() it before
        free())"""
        img = np.ascontiguousarray(panorama_rgba8, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError("a panorama is (height, width, 4) uint8")
        o = self.sky_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_sky_create(self.context, _ref(o), img.ctypes.data, img.shape[1], img.shape[0], C.byref(out)))
        return Sky(out, img.shape[1], img.shape[0])

    def sky_destroy(self, sky):
        self._destroy(sky, self._lib.ow_sky_destroy)

    def environment_apply(self, camera, pixels, sky=None, options=None):
        """Sky fill and fog over `pixels` ((H, W) RENDER_PIXEL records of the draws): the records with color and status rewritten (a copy).
        Synchronises."""
        o = self.environment_options(options)
        _, rec = self._picture(camera, pixels, False)
        _lib.check(self._lib.ow_environment_apply(self.context, _handle(sky), C.byref(camera), _ref(o), rec.ctypes.data))
        return rec

    def environment_apply_async(self, camera, pixels_device, sky=None, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, None, pixels_device)
        o = self.environment_options(options)
        _lib.check(self._lib.ow_environment_apply_async(self.context, _handle(sky), C.byref(camera), _ref(o), _addr(pixels_device)))

    @classmethod
    def present_size(cls, camera, options=None):
        """(height, width) of what present() returns for records of the camera's size"""
        o = cls.present_options(options)
        s = max(int(o.downsample), 1) if o is not None else 1
        return int(camera.height) // s, int(camera.width) // s

    def present(self, camera, pixels, options=None, linear=False):
        """The finished picture of `pixels` ((H, W) RENDER_PIXEL records; camera.width x camera.height is THEIR size): (H / s, W / s, 4) uint8 sRGB
        RGBA, or with linear=True the pair (RGBA, (H / s, W / s, 4) float32 resolved linear RGB and hit share).  Synchronises."""
        o = self.present_options(options)
        _, rec = self._picture(camera, pixels, False)
        h, w = self.present_size(camera, o)
        rgba = np.zeros((max(h, 1), max(w, 1), 4), np.uint8)
        lin = np.zeros((max(h, 1), max(w, 1), 4), np.float32) if linear else None
        _lib.check(self._lib.ow_present(self.context, C.byref(camera), _ref(o), rec.ctypes.data, rgba.ctypes.data, _data(lin)))
        return (rgba, lin) if linear else rgba

    def present_async(self, camera, pixels_device, rgba_device, linear_device=None, options=None):
        """The present over DEVICE buffers, enqueued in the generator's stream order without synchronising: pixels_device holds the camera's
        H * W records, rgba_device (H / s) * (W / s) * 4 bytes, linear_device as many float4; either output may be None (not both)"""
        o = self.present_options(options)
        h, w = self.present_size(camera, o)
        _check_device_size(pixels_device, int(camera.width) * int(camera.height), self.RENDER_PIXEL.itemsize, "pixels_device", "records")
        _check_device_size(rgba_device, h * w, 4, "rgba_device", "pixels")
        _check_device_size(linear_device, h * w, 16, "linear_device", "pixels")
        _lib.check(self._lib.ow_present_async(self.context, C.byref(camera), _ref(o), _addr(pixels_device), _addr(rgba_device, True),
                                              _addr(linear_device, True)))

    # ---- the sky's light: the roughness-blurred pyramid and the irradiance (include/ocean_waves.h ow_radiance_*) ----
    _RADIANCE_OWN = ("levels", "samples", "base_width")
    _SKY_LIGHT_OWN = ("ambient_energy", "reflection_energy", "specular")

    @classmethod
    def radiance_options(cls, options=None):
        """None, an _lib.ow_radiance_options, or a dict of levels, samples and base_width over ow_radiance_options_default's values"""
        return cls._options(_lib.ow_radiance_options, _lib.load().ow_radiance_options_default, cls._RADIANCE_OWN, options, "radiance")

    @classmethod
    def sky_light_options(cls, options=None):
        """None, an _lib.ow_radiance_light_options, or a dict of ambient_energy, reflection_energy and specular over
        ow_radiance_light_options_default's values (1, 1, 0.5)"""
        return cls._options(_lib.ow_radiance_light_options, _lib.load().ow_radiance_light_options_default, cls._SKY_LIGHT_OWN, options, "sky light")

    def radiance_create(self, sky, options=None):
        """The roughness-blurred pyramid and the irradiance of a Sky, built once on the device; returns a Radiance (radiance_destroy() it
        before free()).  The sky may be destroyed afterwards."""
        o = self.radiance_options(options)
        out, n = C.c_void_p(), C.c_int32()
        _lib.check(self._lib.ow_radiance_create(self.context, sky.handle, _ref(o), C.byref(out)))
        _lib.check(self._lib.ow_radiance_level(self.context, out, 0, C.byref(n), None, None, None))
        return Radiance(out, n.value)

    def radiance_destroy(self, radiance):
        self._destroy(radiance, self._lib.ow_radiance_destroy)

    def radiance_level(self, radiance, level):
        """(H, W, 4) float32 texels of level `level` (0 .. levels - 1), or of the 16 x 32 irradiance with level="irradiance".  Synchronises."""
        k = _lib.OW_RADIANCE_IRRADIANCE if level == "irradiance" else int(level)
        w, h = C.c_int32(), C.c_int32()
        _lib.check(self._lib.ow_radiance_level(self.context, radiance.handle, k, None, C.byref(w), C.byref(h), None))
        out = np.zeros((h.value, w.value, 4), np.float32)
        _lib.check(self._lib.ow_radiance_level(self.context, radiance.handle, k, None, None, None, out.ctypes.data))
        return out

    def sky_light_apply(self, radiance, camera, pixels, options=None):
        """Sky ambient and sky reflection over `pixels` ((H, W) RENDER_PIXEL records of the draws, made with ambient_color 0): the records
        with color and status rewritten (a copy).  Call it before environment_apply.  Synchronises."""
        o = self.sky_light_options(options)
        _, rec = self._picture(camera, pixels, False)
        _lib.check(self._lib.ow_radiance_light_apply(self.context, _handle(radiance), C.byref(camera), _ref(o), rec.ctypes.data))
        return rec

    def sky_light_apply_async(self, radiance, camera, pixels_device, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, None, pixels_device)
        o = self.sky_light_options(options)
        _lib.check(self._lib.ow_radiance_light_apply_async(self.context, _handle(radiance), C.byref(camera), _ref(o), _addr(pixels_device)))
