"""MI355X-native drop-in for the wave-generation hot path of 2Retr0/GodotOceanWaves.

The product is godotoceanwaves_amd/libocean_waves.so (hand-written HIP for gfx950 behind the C-ABI in
include/ocean_waves.h).  This package is the host-side mirror of the reference's
`WaveGenerator` / `WaveCascadeParameters` interface on top of that ABI (wave_generator.py), and of what a consumer
does with the maps: one module of wrapper calls per read-side unit of the library (_points, _bodies, _mesh, _spray,
_solid, _sky), the debug surface (_lab) and their shared helpers (_shared).  No numerics live here.
"""
from .wave_generator import Sky, WaveCascadeParameters, WaveGenerator  # noqa: F401
from .group import WaveGeneratorGroup  # noqa: F401
from .presets import cascade_preset, DEPTH, UPDATE_DELTA  # noqa: F401
