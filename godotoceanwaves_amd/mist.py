"""Height mist with sun shafts over camera pictures on the device (csrc/ow_mist_host.hip, include/ocean_waves.h ow_mist_*): functions over
a live WaveGenerator and the ShadowMap its shadow_map_create returns.  The pass goes after environment_apply and before spray_draw."""
import ctypes as C

from . import _lib
from ._shared import _addr, _data, _handle, _ref, _stats, Shared

_OWN = ("extinction", "height_falloff", "base_height", "length", "anisotropy", "sky_affect", "slices", "shadow_bias", "albedo", "sun_color",
        "sun_direction", "ambient_color")


def mist_options(options=None):
    """None, an _lib.ow_mist_options, or a dict over ow_mist_options_init's values (the reference scene's sea mist: height_falloff 0.176,
    length 256, the scene's sun) that may set extinction, height_falloff, base_height, length, anisotropy, sky_affect, slices, shadow_bias,
    albedo, sun_color, sun_direction and ambient_color"""
    return Shared._options(_lib.ow_mist_options, _lib.load().ow_mist_options_init, _OWN, options, "mist")


def mist_apply(gen, camera, pixels, shadow_map=None, options=None, rgba=False):
    """The mist laid over `pixels` ((H, W) RENDER_PIXEL records, environment_apply's), with the shafts of shadow_map's casters cut out of it
    where one is given: (the (H, W, 4) uint8 RGBA image or None, the records with status and color rewritten (a copy)).  Synchronises."""
    o = mist_options(options)
    img, rec = Shared._picture(camera, pixels, rgba)
    _lib.check(gen._lib.ow_mist_apply(gen.context, _handle(shadow_map), C.byref(camera), _ref(o), rec.ctypes.data, _data(img)))
    return img, rec


def mist_apply_async(gen, camera, pixels_device, shadow_map=None, rgba_device=None, options=None):
    """The pass over DEVICE records, in place, enqueued in the generator's stream order without synchronising"""
    gen._check_picture_buffers(camera, rgba_device, pixels_device)
    o = mist_options(options)
    _lib.check(gen._lib.ow_mist_apply_async(gen.context, _handle(shadow_map), C.byref(camera), _ref(o), _addr(pixels_device), _addr(rgba_device, True)))


def mist_stats(gen, counters=True):
    """dict of the passes enqueued and, with counters (synchronising), over the last pass the pixels processed, the slices whose depth
    compare read the map and the slices found shadowed"""
    return _stats(gen._lib.ow_mist_stats, (gen.context,), ("passes", "pixels", "slices_fetched", "slices_shadowed"),
                  () if counters else ("pixels", "slices_fetched", "slices_shadowed"))
