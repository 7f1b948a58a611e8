"""The floating bodies reflected in the water of camera pictures on the device (csrc/ow_mirror_host.hip, include/ocean_waves.h ow_mirror_*):
functions over a live WaveGenerator, the Radiance its radiance_create returns and the handle objects of solid_create and bodies_create.  The
pass takes radiance_light_apply's place: after shadow_apply and before environment_apply."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _check_device_size, _data, _handle, _ref, _rest, _stats, Shared
from .solid_cast import SOLID_HIT

_OWN = ("ambient_energy", "reflection_energy", "specular", "body_color", "light_direction", "light_color", "ambient_color", "max_distance",
        "fade_begin", "opacity", "cull", "two_sided")
_COUNTERS = ("pixels", "rays_cast", "sphere_tests_passed", "pairs_tested", "rays_hit")


def mirror_options(options=None):
    """None, an _lib.ow_mirror_options, or a dict over ow_mirror_options_init's values (the sky pass's energies, the solid draw's colours and
    sun, 200 m of mirror ray fading out from 100 m, opacity 1) that may set ambient_energy, reflection_energy, specular, body_color,
    light_direction, light_color, ambient_color, max_distance, fade_begin, opacity, cull (0, or -1: no culling, for measurements) and
    two_sided"""
    o = Shared._options(_lib.ow_mirror_options, _lib.load().ow_mirror_options_init, _OWN, options, "mirror")
    if o is not options and options.get("two_sided"):
        o.flags |= _lib.OW_MIRROR_TWO_SIDED
    return o


def _host(camera, pixels, hits):
    _, rec = Shared._picture(camera, pixels, False)
    return rec, (np.zeros(rec.shape, SOLID_HIT) if hits else None)


def mirror_apply(gen, radiance, camera, pixels, solid=None, bodies_set=None, options=None, first=0, count=None, hits=False):
    """The sky's light and the bodies' reflections added to `pixels` ((H, W) RENDER_PIXEL records, shadow_apply's), against bodies [first,
    first + count) of a set at their resident poses (no solid and no set: the pass is radiance_light_apply): the records with color and
    status rewritten (a copy), or with hits (the records, the (H, W) SOLID_HIT records of the mirror rays).  Synchronises."""
    o = mirror_options(options)
    rec, out = _host(camera, pixels, hits)
    n = 0 if bodies_set is None else _rest(bodies_set, first, count)
    _lib.check(gen._lib.ow_mirror_apply(gen.context, radiance.handle, _handle(solid), _handle(bodies_set), int(first), int(n), C.byref(camera), _ref(o),
                                        rec.ctypes.data, _data(out)))
    return (rec, out) if hits else rec


def mirror_apply_instances(gen, radiance, camera, pixels, solid, transforms, options=None, hits=False):
    """mirror_apply over a host array of [count][12] transforms (basis rows, then the origin)"""
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
    o = mirror_options(options)
    rec, out = _host(camera, pixels, hits)
    _lib.check(gen._lib.ow_mirror_apply_instances(gen.context, radiance.handle, _handle(solid), t.ctypes.data if len(t) else None, len(t), C.byref(camera),
                                                  _ref(o), rec.ctypes.data, _data(out)))
    return (rec, out) if hits else rec


def mirror_apply_async(gen, radiance, camera, pixels_device, solid=None, bodies_set=None, hits_device=None, options=None, first=0, count=None):
    """The pass over DEVICE records, in place, and optionally into DEVICE SOLID_HIT records, enqueued in the generator's stream order without
    synchronising"""
    gen._check_picture_buffers(camera, None, pixels_device)
    if hits_device is not None:
        _check_device_size(hits_device, int(camera.width) * int(camera.height), SOLID_HIT.itemsize, "hits_device")
    o = mirror_options(options)
    n = 0 if bodies_set is None else _rest(bodies_set, first, count)
    _lib.check(gen._lib.ow_mirror_apply_async(gen.context, radiance.handle, _handle(solid), _handle(bodies_set), int(first), int(n), C.byref(camera),
                                              _ref(o), _addr(pixels_device), _addr(hits_device, True)))


def mirror_stats(gen, counters=True):
    """dict of the passes enqueued and, with counters (synchronising), over the last pass the pixels processed, the mirror rays cast, the
    sphere tests they passed, the (ray, triangle) pairs tested and the rays that met a body"""
    return _stats(gen._lib.ow_mirror_stats, (gen.context,), ("passes",) + _COUNTERS, () if counters else _COUNTERS)
