"""examples/scene.h against tests/scenes.py, on the CPU: the example programs take their crates, box, clip-map grid, panorama and spray
textures from the header, and their GPU tests hand the wrapper scenes.py's restatements of them and compare the finished pictures byte for
byte.  Here the two are held to each other directly: tests/example_scene/scene_dump.c runs the header's generators on their own (C99,
-Wall -Wextra -pedantic -Werror, the address and undefined-behaviour sanitizers, nothing of the library linked) and writes their arrays
raw; every array is the bytes scenes.py makes."""
import subprocess

import numpy as np

from cpu_builds import build_scene_dump
from scenes import box, CRATE_SHAPE, example_crates, example_panorama, example_textures, grid


def test_the_headers_generators_write_the_bytes_of_scenes_py(tmp_path):
    exe = build_scene_dump(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "cells=128 cell=4 crates=36 per_crate=32 panorama=256x128 textures=64x64\n"
    states, hull = example_crates()
    box_vertices, box_triangles = box(CRATE_SHAPE)
    grid_vertices, grid_triangles = grid(128, 4.0)
    albedo, dissolve = example_textures()
    want = dict(crate_states=states, crate_hull=hull, box_vertices=box_vertices, box_triangles=box_triangles, grid_vertices=grid_vertices,
                grid_triangles=grid_triangles, panorama=example_panorama(), albedo=albedo, dissolve=dissolve)
    kinds = dict(box_vertices=np.float32, grid_vertices=np.float32, box_triangles=np.int32, grid_triangles=np.int32, panorama=np.uint8,
                 albedo=np.uint8, dissolve=np.uint8)
    for name, array in want.items():
        assert array.dtype == kinds.get(name, array.dtype), name     # as made, not after a conversion: the wrapper's would be a no-op
        got = (tmp_path / (name + ".bin")).read_bytes()
        assert len(got) == array.nbytes and got == array.tobytes(), name
