"""The wrapper's debug and measurement surface: what the tests and the benchmark read out of a context beyond its maps -- the push constants,
the FP32 maps, the spectrum and the intermediate, the test hooks, the scheduler's last_* and *_stats, the timers and the kernel probe
(include/ocean_waves.h's debug entry points; csrc/ow_schedule.hip keeps the counters)."""
import ctypes as C

import numpy as np

from . import _lib
from ._shared import _data


class LabCalls:
    def debug_inject_fault(self, bits):
        """test hook (ow_debug_inject_fault): fault bits for the next batch only"""
        _lib.check(self._lib.ow_debug_inject_fault(self.context, int(bits)))

    def sync_stats(self):
        """stream synchronisations the library has made on this thread since init_gpu (ow_sync_stats); does not synchronise"""
        v = C.c_uint64()
        _lib.check(self._lib.ow_sync_stats(self.context, C.byref(v)))
        return v.value

    def get_push_constants(self, cascade):
        """(spectrum[16], modulate[8], unpack[4]) uint32 words: the reference's push-constant blocks of this cascade's most recent launch"""
        pc = _lib.ow_push_constants()
        _lib.check(self._lib.ow_get_push_constants(self.context, cascade, C.byref(pc)))
        return (np.array(pc.spectrum, np.uint32), np.array(pc.modulate, np.uint32), np.array(pc.unpack, np.uint32))

    def get_maps_f32(self, cascade):
        out = np.empty((self.map_size, self.map_size, 8), np.float32)
        _lib.check(self._lib.ow_get_maps_f32(self.context, cascade, out.ctypes.data))
        return out

    def get_spectrum(self, cascade):
        n = self.map_size
        h0, om = np.empty((n, n, 4), np.float32), np.empty((n, n), np.float32)
        _lib.check(self._lib.ow_get_spectrum(self.context, cascade, h0.ctypes.data, om.ctypes.data))
        return h0, om

    def debug_set_spectrum(self, cascade, h0, omega=None):
        """test hook (ow_debug_set_spectrum): h0 complex64 [n][n] = h0(k) as [y][x] replaces the resident spectrum of `cascade`; omega float32
        [n][n] replaces its dispersion plane (None keeps it)"""
        n = self.map_size
        h0 = np.ascontiguousarray(h0, np.complex64)
        if h0.shape != (n, n):
            raise ValueError(f"h0 must be [{n}][{n}], got {h0.shape}")
        if omega is not None:
            omega = np.ascontiguousarray(omega, np.float32)
            if omega.shape != (n, n):
                raise ValueError(f"omega must be [{n}][{n}], got {omega.shape}")
        _lib.check(self._lib.ow_debug_set_spectrum(self.context, cascade, h0.ctypes.data, _data(omega)))

    def get_intermediate(self, cascade):
        out = np.empty((4, self.map_size, self.map_size, 2), np.float32)
        _lib.check(self._lib.ow_get_intermediate(self.context, cascade, out.ctypes.data))
        return out

    KERNEL_FAMILIES = {0: None, 1: "standard", 2: "layer_parallel", 3: "compact", 4: "layer_parallel_compact", 5: "tick_groups_compact",
                       6: "tick_pairs_compact"}

    def last_kernel_family(self):
        """which kernels the most recent batch ran with: "standard", "layer_parallel", "compact" (None before the first launch)"""
        return self.KERNEL_FAMILIES[int(self._lib.ow_last_kernel_family(self.context))]

    def last_batch_cascades(self):
        """cascades in the most recent pair of launches (a tick may be split into several pairs)"""
        return int(self._lib.ow_last_batch_cascades(self.context))

    def tick_group_depth(self):
        """ticks per launch: of the most recent run() that went out in tick groups / tick pairs, else the depth planned for this
        context's small batches (0: no tick groups)"""
        return int(self._lib.ow_tick_group_depth(self.context))

    def lookahead_stats(self):
        """(hits, speculated): update_all() ticks whose pass 1 had been speculated by the previous call, and speculations launched"""
        h, sp = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_lookahead_stats(self.context, C.byref(h), C.byref(sp)))
        return h.value, sp.value

    def chain_stats(self):
        """launches that went out as two chains on two streams (1024^2, four cascades a side; OW_FLAG_SINGLE_STREAM keeps them whole)"""
        n = C.c_uint64()
        _lib.check(self._lib.ow_chain_stats(self.context, C.byref(n)))
        return n.value

    def spectrum_stats(self):
        """(generated, skipped): spectrum kernels launched, and dirty flags consumed because the resident spectrum had been generated from the
        same thirteen packed constants (a whitecap / foam_amount edit: wave_cascade_parameters.gd:32-35 raise the flag, spectrum_compute never reads them)"""
        g, sk = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_spectrum_stats(self.context, C.byref(g), C.byref(sk)))
        return g.value, sk.value

    def timing(self, enable):
        """False / 0: off; True / 1: per pass (run() stays on one launch per pass); 2: as launched (tick groups / pairs stay on and are
        timed per launch: timing_read_launches)"""
        _lib.check(self._lib.ow_timing_enable(self.context, 2 if enable == 2 else (1 if enable else 0)))

    def probe_kernel_times(self, reps=50):
        """(pass1_ms, pass2_ms, cascades_per_launch): each kernel alone, `reps` back-to-back launches (benchmark probe;
        the extra pass-2 launches advance the foam state)"""
        a, b, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_probe_kernel_times(self.context, reps, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def timing_read_launches(self, reset=True):
        """(average ms, count) of the tick-group / tick-pair launches timed under timing(2)"""
        a, n = C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_timing_read_launches(self.context, C.byref(a), C.byref(n), 1 if reset else 0))
        return a.value, n.value

    def timing_read(self, reset=True):
        a, b, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_timing_read(self.context, C.byref(a), C.byref(b), C.byref(n), 1 if reset else 0))
        return a.value, b.value, n.value
