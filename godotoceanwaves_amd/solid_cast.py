"""Ray casts against the floating bodies on the device (csrc/ow_solid_host.hip, include/ocean_waves.h ow_cast_*): functions over a
live WaveGenerator and the handle objects its solid_create and bodies_create return."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _addr, _check_device_size, _count, _data, _ref, _rest, _stats, Shared

SOLID_HIT = np.dtype(_lib.ow_solid_hit)
_OWN = ("two_sided", "cull")


def solid_cast_options(options=None):
    """None, an _lib.ow_solid_cast_options, or a dict over zeros, the defaults (one-sided, culled by bounding spheres), that
    may set two_sided and cull (0: the default; -1: no culling, for measurements)"""
    o = Shared._options(_lib.ow_solid_cast_options, None, _OWN, options, "solid cast")
    if o is not options and options.get("two_sided"):
        o.flags |= _lib.OW_SOLID_CAST_TWO_SIDED
    return o


def _host_rays(rays, water_hits):
    r = np.ascontiguousarray(rays, Shared.RAY).reshape(-1)
    w = None
    if water_hits is not None:
        w = np.ascontiguousarray(water_hits, Shared.RAYCAST_HIT).reshape(-1)
        if len(w) != len(r):
            raise ValueError(f"water_hits holds {len(w)} records for {len(r)} rays")
    return r, w, np.zeros(len(r), SOLID_HIT)


def raycast_solids(gen, solid, bodies_set, rays, water_hits=None, options=None, first=0, count=None):
    """Where each ray (RAY records: WaveGenerator.rays) first meets the shape at the resident poses of bodies [first, first + count) of a body
    set: SOLID_HIT records.  water_hits: raycast_surface's records for the same rays; a solid then counts only when it is no farther than
    the water.  Synchronises."""
    r, w, out = _host_rays(rays, water_hits)
    o = solid_cast_options(options)
    _lib.check(gen._lib.ow_cast_bodies(gen.context, solid.handle, bodies_set.handle, int(first), int(_rest(bodies_set, first, count)), _data(r), len(r),
                                          _data(w), _ref(o), _data(out)))
    return out


def raycast_solids_instances(gen, solid, transforms, rays, water_hits=None, options=None):
    """raycast_solids over a host array of [count][12] transforms (basis rows, then the origin)"""
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
    r, w, out = _host_rays(rays, water_hits)
    o = solid_cast_options(options)
    _lib.check(gen._lib.ow_cast_instances(gen.context, solid.handle, t.ctypes.data if len(t) else None, len(t), _data(r), len(r), _data(w), _ref(o),
                                                    _data(out)))
    return out


def raycast_solids_async(gen, solid, bodies_set, rays_device, out_device, water_hits_device=None, options=None, first=0, count=None, ray_count=None):
    """The cast over DEVICE buffers (rays, SOLID_HIT records out, optionally raycast_surface_async's records), enqueued in the generator's
    stream order without synchronising.  ray_count: the number of rays, needed for raw addresses"""
    n = _count(ray_count, rays_device, Shared.RAY, "ray_count")
    _check_device_size(out_device, n, SOLID_HIT.itemsize)
    if water_hits_device is not None:
        _check_device_size(water_hits_device, n, Shared.RAYCAST_HIT.itemsize, "water_hits_device")
    o = solid_cast_options(options)
    _lib.check(gen._lib.ow_cast_bodies_async(gen.context, solid.handle, bodies_set.handle, int(first), int(_rest(bodies_set, first, count)),
                                                _addr(rays_device), n, _addr(water_hits_device, True), _ref(o), _addr(out_device)))


def raycast_solids_stats(gen, counters=True):
    """dict of casts, the scratch bytes held and, with counters (synchronising), the instances the last cast skipped, and summed over its valid
    rays the instances that passed the sphere test and the (instance, triangle) pairs tested"""
    return _stats(gen._lib.ow_cast_stats, (gen.context,), ("casts", "skipped_instances", "sphere_tests_passed", "pairs_tested", "scratch_bytes"),
                  () if counters else ("skipped_instances", "sphere_tests_passed", "pairs_tested"))
