"""The four handle kinds of the read side -- body sets, meshes, spray emitters, billboard materials -- share one base, one list on their
context and one life cycle (godotoceanwaves_amd/csrc/ow_context.h ow::Handle).  The per-feature tests hold one kind at a time; here every kind
lives on one context at once, at the smallest shapes: each create and each destroy costs exactly one stream synchronisation, a destroy leaves
the other kinds usable, handles that outlive their context are orphans (refused by every call, still destroyable), creation-order destroys
work, and a handle is refused by a context that does not own it.
"""
import ctypes as C

import numpy as np
import pytest

from godotoceanwaves_amd import WaveCascadeParameters, _lib
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W

KINDS = ("material", "emitter", "mesh", "bodies")


def context():
    """map size 128, 2 cascades, one run of 1 tick -> (generator, map_scales)"""
    gen = W()
    gen.map_size = 128
    gen.init_gpu(2)
    params = [WaveCascadeParameters(tile_length=(88.0, 88.0)), WaveCascadeParameters(tile_length=(57.0, 57.0), spectrum_seed=(3, 5))]
    gen.run(UPDATE_DELTA, params, 1)
    return gen, np.array([(1 / p.tile_length[0], 1 / p.tile_length[1], p.displacement_scale, p.normal_scale) for p in params], np.float32)


def two_bodies():
    """2 bodies of 8 hull points each"""
    hull = np.concatenate([W.box_hull((2.0, 1.0, 2.0), (2, 2, 2), body=b) for b in range(2)])
    st = np.zeros(2, W.RIGID_BODY)
    mass, iinv = W.box_mass_properties((2.0, 1.0, 2.0), 500.0)
    for b in range(2):
        st[b]["position"] = (10.0 * b, 0.0, 0.0)
        st[b]["orientation"] = (0, 0, 0, 1)
        st[b]["mass"], st[b]["inverse_inertia"] = mass, iinv
        st[b]["point_offset"], st[b]["point_count"] = 8 * b, 8
    return st, hull


CREATE = {
    "bodies": lambda gen: gen.bodies_create(*two_bodies()),
    "mesh": lambda gen: gen.mesh_create([(0, 0, 0), (1, 0, 0), (0, 0, 1)], [(0, 2, 1)]),          # one triangle
    "emitter": lambda gen: gen.spray_create({"amount": _lib.OW_SPRAY_MIN_AMOUNT}),
    "material": lambda gen: gen.spray_material_create(np.full((1, 1, 4), 255, np.uint8), np.zeros((1, 1, 4), np.uint8)),   # two 1 x 1 textures
}
DESTROY = {"bodies": W.bodies_destroy, "mesh": W.mesh_destroy, "emitter": W.spray_destroy, "material": W.spray_material_destroy}


def camera():
    return W.camera((0.0, 5.0, 0.0), np.eye(3), 90.0, 8, 8, 1000.0)


def counted(gen, fn, *args):
    """fn(gen, *args) and the stream synchronisations it cost"""
    before = gen.sync_stats()
    out = fn(gen, *args)
    return out, gen.sync_stats() - before


def call_with(lib, ctx, kind, handle):
    """one call per kind whose last check is the handle's against `ctx` -> (status, ow_last_error)"""
    h = handle.handle
    if kind == "bodies":
        code = lib.ow_bodies_get_device_ptrs(ctx, h, None, None, None)
    elif kind == "mesh":
        code = lib.ow_mesh_get_device_ptrs(ctx, h, None, None)
    elif kind == "emitter":
        code = lib.ow_spray_get_device_ptrs(ctx, h, None, None, None, None)
    else:
        rgba = np.zeros((8, 8, 4), np.uint8)
        code = lib.ow_billboard_draw_instances(ctx, h, None, 0, 0.0, C.byref(camera()), None, None, rgba.ctypes.data)
    return code, lib.ow_last_error()


@pytest.mark.gpu
def test_every_kind_on_one_context_and_orphans():
    gen, sc = context()
    lib = gen._lib
    h = {}
    for kind in ("bodies", "mesh", "emitter", "material"):
        h[kind], syncs = counted(gen, CREATE[kind])
        assert syncs == 1, (kind, syncs)
    for kind in ("mesh", "bodies"):              # the emitter and the material live on
        _, syncs = counted(gen, DESTROY[kind], h[kind])
        assert syncs == 1 and not h[kind].handle, (kind, syncs)
    cam = camera()
    gen.spray_step(h["emitter"], UPDATE_DELTA, sc)
    rgba, rec = gen.spray_draw(h["emitter"], h["material"], cam)
    assert rgba.shape == (8, 8, 4) and rec is None
    assert gen.spray_draw_stats()["draws"] == 1
    gen.free()                                    # the emitter and the material are orphans now
    assert gen.context is None
    for kind in ("emitter", "material"):
        code, msg = call_with(lib, None, kind, h[kind])
        assert code == _lib.OW_ERR_INVALID and b"null context" in msg, (kind, code, msg)
        DESTROY[kind](gen, h[kind])               # *_destroy(NULL, handle): the orphan's own memory only
        assert not h[kind].handle


@pytest.mark.gpu
def test_destroys_in_creation_order():
    gen, _ = context()
    h = {}
    for kind in KINDS:
        h[kind], syncs = counted(gen, CREATE[kind])
        assert syncs == 1, (kind, syncs)
    for kind in KINDS:                            # creation order, not the reverse
        _, syncs = counted(gen, DESTROY[kind], h[kind])
        assert syncs == 1, (kind, syncs)
    gen.sync()
    gen.free()


@pytest.mark.gpu
def test_a_handle_is_refused_by_another_context():
    gen, _ = context()
    other, _ = context()
    for kind in KINDS:
        mine = CREATE[kind](gen)
        code, msg = call_with(gen._lib, other.context, kind, mine)
        assert code == _lib.OW_ERR_INVALID and b"belongs to another context" in msg, (kind, code, msg)
        if kind != "material":                    # its own context takes it (the material's call would go on to draw)
            assert call_with(gen._lib, gen.context, kind, mine)[0] == _lib.OW_OK, kind
        DESTROY[kind](gen, mine)
    other.free()
    gen.free()
