"""Floating bodies stepped on the device (csrc/ow_bodies_host.hip, include/ocean_waves.h ow_bodies_*)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _BodySet, _ref, _rest, _scales, _stats, Shared


class BodiesCalls(Shared):
    @staticmethod
    def box_mass_properties(size, density):
        """(mass, inverse principal inertia) of a solid box of size (x, y, z) metres and uniform density (kg/m^3) about its centre"""
        sx, sy, sz = (float(v) for v in size)
        mass = density * sx * sy * sz
        inertia = (mass / 12.0 * (sy * sy + sz * sz), mass / 12.0 * (sx * sx + sz * sz), mass / 12.0 * (sx * sx + sy * sy))
        return mass, tuple(1.0 / i for i in inertia)

    @classmethod
    def bodies_options(cls, options=None):
        """None, an _lib.ow_bodies_options, or what buoyancy_options() (_points.py) takes -> ow_bodies_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_bodies_options):
            return options
        return _lib.ow_bodies_options(buoyancy=cls.buoyancy_options(options))

    def bodies_create(self, bodies, hull):
        """A device-resident body set from RIGID_BODY records and HULL_POINT records; returns a _BodySet (bodies_destroy() it before free())"""
        b = np.ascontiguousarray(bodies, self.RIGID_BODY)
        h = np.ascontiguousarray(hull, self.HULL_POINT)
        out = C.c_void_p()
        _lib.check(self._lib.ow_bodies_create(self.context, b.ctypes.data, len(b), h.ctypes.data, len(h), C.byref(out)))
        return _BodySet(out, len(b), len(h))

    def bodies_destroy(self, bodies_set):
        self._destroy(bodies_set, self._lib.ow_bodies_destroy)

    def bodies_step(self, bodies_set, map_scales, substeps, dt, options=None):
        """`substeps` substeps of dt seconds, enqueued in the generator's stream order without synchronising"""
        sc = _scales(map_scales)
        o = self.bodies_options(options)
        _lib.check(self._lib.ow_bodies_step(self.context, bodies_set.handle, sc.ctypes.data, len(sc), _ref(o), int(substeps),
                                            float(dt)))

    def bodies_state(self, bodies_set, first=0, count=None):
        """RIGID_BODY records of bodies [first, first + count) (count None: up to the last one); synchronises"""
        out = np.zeros(_rest(bodies_set, first, count), self.RIGID_BODY)
        _lib.check(self._lib.ow_bodies_get_state(self.context, bodies_set.handle, int(first), len(out), out.ctypes.data))
        return out

    def bodies_set_state(self, bodies_set, records, first=0):
        r = np.ascontiguousarray(records, self.RIGID_BODY)
        _lib.check(self._lib.ow_bodies_set_state(self.context, bodies_set.handle, int(first), len(r), r.ctypes.data))

    def bodies_results(self, bodies_set, first=0, count=None):
        """BUOYANCY_RESULT records of the last substep; synchronises"""
        out = np.zeros(_rest(bodies_set, first, count), self.BUOYANCY_RESULT)
        _lib.check(self._lib.ow_bodies_get_results(self.context, bodies_set.handle, int(first), len(out), out.ctypes.data))
        return out

    def bodies_device_ptrs(self, bodies_set):
        """device addresses of the pose records (BUOYANCY_BODY, Transform3D layout), the results and the per-point records"""
        b, r, p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.ow_bodies_get_device_ptrs(self.context, bodies_set.handle, C.byref(b), C.byref(r), C.byref(p)))
        return b.value, r.value, p.value

    def bodies_stats(self, bodies_set, faulted=True):
        """dict of substeps, fused_launches, split_calls and (synchronising) faulted_bodies"""
        return _stats(self._lib.ow_bodies_stats, (self.context, bodies_set.handle), ("substeps", "fused_launches", "split_calls", "faulted_bodies"),
                      () if faulted else ("faulted_bodies",))
