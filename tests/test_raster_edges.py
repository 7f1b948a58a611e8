"""The walk of the three triangle draws (csrc/ow_raster.h raster_wave under k_mesh_raster, k_solid_raster and k_shadow_raster; the set-ups'
boxes of ow_mesh.h tri_setup and ow_shadow.h shadow_setup) against brute-force coverage: the harnesses' harness_*_cover_all test every
triangle that facing, flags and det do not cull at EVERY centre of the picture or map, whatever the set-up made of its box, and the boxed
CPU builds and the device must write the same words.  The inputs (tests/raster_soups.py) are placed on the walk's edges -- a box of exactly
lane_box and lane_box + 1 centres, box edges at 8 k - 1, 8 k and 8 k + 1, boxes clamped at the last column of a picture that is no
multiple of 8, one-centre boxes in the corners, the wave class alone in lane 0 or lane 63 or in every lane or in the last lane of a
partial wave, ties between waves, 4 096 layers on one word -- and every such property is asserted from the returned set-ups, so a changed
constant cannot silently empty a case.  Nothing here has a tolerance: words byte for byte, counts exactly.

The closed sheets' claim (ow_mesh.h: a centre on a shared edge is inside one triangle or both, never neither) is exact per edge; at a
vertex where several rounded edge lines meet it is no proof, so what is asserted there is what the CPU build does on these fixed seeds."""
import os

import numpy as np
import pytest

import mesh_twin
import raster_soups as RS
from checks import assert_same_picture, same_picture
from cpu_builds import mesh_harness, shadow_harness, solid_harness  # noqa: F401 (fixtures)
from raster_soups import LANE, LANE_BOXES, ONE_ORIGIN, TARGETS, WAVE
from scenes import NEAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = os.path.join(ROOT, "profiles", "raster_edges.txt")
NAMES = ("mesh", "solid", "shadow")
LOW = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def builds(mesh_harness, solid_harness, shadow_harness):  # noqa: F811
    return {"mesh": mesh_harness, "solid": solid_harness, "shadow": shadow_harness}


def ids_of(words):
    return (words & LOW).astype(np.int64)


def depth_halves(target, words):
    return words >> np.uint64(32) if target.name != "shadow" else words


def boxed_is_brute(target, L, V, origins, size, lane_boxes, what):
    """the boxed CPU build at every lane_box against one brute pass: the words, the lane + wave count, the picture resolved from the words,
    and no covered centre outside a set-up's box, occluded triangles included.  Returns the brute pass."""
    brute = target.cpu(L, V, origins, size, lane_boxes[0], brute=True)
    assert int(brute["cover"]["outside"].sum()) == 0, (what, "covered centres outside their box", np.flatnonzero(brute["cover"]["outside"])[:8])
    assert not brute["cover"]["covered"][brute["setups"]["kind"] < LANE].any(), (what, "a covering triangle is not drawn")
    for lane_box in lane_boxes:
        boxed = target.cpu(L, V, origins, size, lane_box)
        assert boxed["words"].tobytes() == brute["words"].tobytes(), (what, lane_box, "words")
        assert boxed["drawn"] == brute["drawn"] == int((brute["setups"]["kind"] >= LANE).sum()), (what, lane_box, "lane + wave")
        if boxed["rec"] is not None:
            same_picture(boxed, brute, (what, lane_box))
    return brute


def setups_of(target, L, size, lane_box):
    return lambda V: target.cpu(L, V, ONE_ORIGIN, size, lane_box, brute="setups")


# ---- the cases both sides draw ----------------------------------------------------------------------------------------------------------------

def placed_cases(target, L):
    """(name, V, origins, size, lane_box, the property its set-ups must show)"""
    out = []
    for k, (lane_box, size) in enumerate(((1, target.odd), (4, target.odd), (64, target.large))):
        P = RS.placed_sides(target, setups_of(target, L, size, lane_box), size, lane_box, 100 + k)
        out.append(("sides %d and %d" % (lane_box, lane_box + 1), target.place(P, size), ONE_ORIGIN, size, lane_box, ("sides", lane_box)))
    size = target.odd
    P = RS.placed_edges(target, setups_of(target, L, size, 0), size, 200)
    out.append(("box edges", target.place(P, size), ONE_ORIGIN, size, 0, ("edges",)))
    return out


def reaches(target, L, case):
    """the property a placed case is there for, from the set-ups of the case itself"""
    name, V, origins, size, lane_box, want = case
    s = target.cpu(L, V, origins, size, lane_box, brute="setups")["setups"]
    sx, sy = RS.sides_of(s)
    longer = np.maximum(sx, sy)
    if want[0] == "sides":
        n = want[1]
        assert ((longer == n) & (s["kind"] == LANE)).sum() >= 2 and ((longer == n + 1) & (s["kind"] == WAVE)).sum() >= 2, (target.name, name, longer, s["kind"])
        assert set(longer) == {n, n + 1} and ((sx == n) | (sx == n + 1)).any() and ((sy == n) | (sy == n + 1)).any()
        return
    w, h = size
    assert w % 8 and h % 8
    assert (s["kind"] >= LANE).all()
    for e in ("x0", "x1", "y0", "y1"):
        for r in RS.PLACED_RESIDUES:
            assert (s[e] % 8 == r).any(), (target.name, e, r)
    assert ((s["x1"] == w - 1) & (sx > 2)).any() and ((s["y1"] == h - 1) & (sy > 2)).any()
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        assert ((s["x0"] == x) & (s["x1"] == x) & (s["y0"] == y) & (s["y1"] == y)).any(), (target.name, "corner", x, y)


def layout_cases(target):
    out = []
    for name, (P, origins) in RS.wave_layouts(target.odd, 300).items():
        out.append((name, target.place(P, target.odd), RS.instance_origins(target) if origins is None else origins, target.odd))
    return out


def check_layout(target, L, name, V, origins, size):
    """at the default lane_box: which lanes of which wave hold a set-up for the wave"""
    kind = target.cpu(L, V, origins, size, 0, brute="setups")["setups"]["kind"]
    assert (kind >= LANE).all(), (target.name, name)
    wave = np.flatnonzero(kind == WAVE)
    if name == "64 for the wave":
        assert len(kind) == 64 and len(wave) == 64
    elif name.startswith("lane"):
        assert len(kind) == 64 and list(wave) == [int(name.split()[1])]
    elif name == "43 x 3":
        assert len(kind) == 129 and list(wave) == [42, 85, 128]          # instance 1 is pairs 43 .. 85, instance 2 pairs 86 .. 128: both cross a wave's end
    else:
        count = int(name.split(",")[0])
        assert len(kind) == count and list(wave) == [count - 1]          # lane 62 of a wave of 63; lane 63; lane 0 of a wave of one


def tie_case(target):
    P, origins = RS.ties(target.tie_size, 400)
    return "ties", target.place(P, target.tie_size), origins, target.tie_size


def layer_case(target):
    P, origins = RS.layers(target)
    return "4096 layers", target.place(P, RS.LAYER_SIZE), origins, RS.LAYER_SIZE


def check_ties(target, brute):
    covered = brute["words"] != target.empty
    assert covered.sum() > 50 and (brute["cover"]["covered"] > 0).sum() >= RS.TIE_COPIES * 20
    if target.name != "shadow":
        assert (ids_of(brute["words"][covered]) < RS.TIE_TRIANGLES).all()      # of 100 equal copies, in 68 waves, the first


def check_layers(target, L, V, origins, size, brute):
    assert (brute["cover"]["covered"] == RS.LAYER_SIZE[0] * RS.LAYER_SIZE[1]).all() and len(brute["cover"]) == 4096
    assert (brute["words"] != target.empty).all()
    if target.name != "shadow":
        assert (ids_of(brute["words"]) == 4095).all()
    alone = target.cpu(L, V[-1:], origins[-1:], size, 0, brute=True)           # the depths are the last layer's own
    assert depth_halves(target, brute["words"]).tobytes() == depth_halves(target, alone["words"]).tobytes()


def family_cases(target, size, count, seed):
    return [(name, V, ONE_ORIGIN, size) for name, V in RS.families(target, np.random.default_rng(seed), count, size).items()]


# ---- 1. boxed equals brute ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_random_soups_boxed_is_brute_at_every_size_and_lane_box(builds, name):
    """every family at every picture and map size, lane_box 0, -1, 1 and 64; the families reach what they are named for"""
    target, L = TARGETS[name], builds[name]
    seen = {}
    for k, size in enumerate(target.sizes):
        for fam, V, origins, _ in family_cases(target, size, 600 if size[0] * size[1] < 2000 else 250, 1000 + k):
            brute = boxed_is_brute(target, L, V, origins, size, LANE_BOXES, (name, size, fam))
            kinds = np.bincount(brute["setups"]["kind"], minlength=4)
            seen[fam] = seen.get(fam, 0) + kinds
            print(name, size, fam, "skipped culled lane wave", kinds, "covered", int(brute["cover"]["covered"].sum()))
    for fam, kinds in seen.items():
        assert kinds[LANE] + kinds[WAVE] > 100 and (kinds[LANE] > 0 and kinds[WAVE] > 0 or fam == "sub"), (name, fam, kinds)   # sub-texel: lanes only


@pytest.mark.parametrize("name", NAMES)
def test_placed_triangles_reach_their_edges_and_boxed_is_brute(builds, name):
    target, L = TARGETS[name], builds[name]
    for case in placed_cases(target, L):
        reaches(target, L, case)
        what, V, origins, size, lane_box, _ = case
        brute = boxed_is_brute(target, L, V, origins, size, (lane_box,) + LANE_BOXES, (name, what))
        assert (brute["cover"]["covered"] > 0).sum() >= len(V) // 2, (name, what)


@pytest.mark.parametrize("name", NAMES)
def test_wave_layouts_hold_the_wave_class_where_they_say(builds, name):
    target, L = TARGETS[name], builds[name]
    for what, V, origins, size in layout_cases(target):
        check_layout(target, L, what, V, origins, size)
        brute = boxed_is_brute(target, L, V, origins, size, LANE_BOXES, (name, what))
        assert (brute["cover"]["covered"][brute["setups"]["kind"] == WAVE] > 0).all(), (name, what)      # what the wave takes covers something


@pytest.mark.parametrize("name", NAMES)
def test_ties_go_to_the_smallest_index_and_layers_to_the_last(builds, name):
    target, L = TARGETS[name], builds[name]
    what, V, origins, size = tie_case(target)
    check_ties(target, boxed_is_brute(target, L, V, origins, size, LANE_BOXES, (name, what)))
    what, V, origins, size = layer_case(target)
    check_layers(target, L, V, origins, size, boxed_is_brute(target, L, V, origins, size, LANE_BOXES, (name, what)))


# ---- 2. the order of the triangles ---------------------------------------------------------------------------------------------------------------

def order_cases(target, L):
    size = target.odd if target.name != "shadow" else (64, 64)
    cases = family_cases(target, size, 250, 500)
    cases += [(c[0], c[1], c[2], c[3]) for c in placed_cases(target, L)[3:]]
    cases.append(tie_case(target))
    return cases


@pytest.mark.parametrize("name", NAMES)
def test_the_picture_does_not_depend_on_the_order_of_the_triangles(builds, name):
    """ow_mesh.h: `the same whatever order the triangles come in` -- the depth halves are, and the indices are the brute pass's of that order (where
    two triangles tie on a centre to the bit, as the copies among the placed ones do, the one that comes first)"""
    target, L = TARGETS[name], builds[name]
    for what, V, origins, size in order_cases(target, L):
        halves = {}
        for order, perm in RS.orders(len(V), 600).items():
            brute = boxed_is_brute(target, L, V[perm], origins, size, (0, -1), (name, what, order))
            halves[order] = depth_halves(target, brute["words"])
        assert halves["given"].tobytes() == halves["reversed"].tobytes() == halves["shuffled"].tobytes(), (name, what)


# ---- 3. closed sheets ----------------------------------------------------------------------------------------------------------------------------

def sheet_conditions(target, V, idx, cells, size):
    """on the vertex positions the draw is given: every border vertex projects at least two centres outside, every depth inside the range"""
    V = V.astype(np.float64)
    w, h = size
    if target.name == "shadow":
        u, v, d = V[..., 0] + w / 2, h / 2 - V[..., 2], RS.DEPTH_RANGE - V[..., 1]
        assert (d > 0.5).all() and (d < 1.95 * RS.DEPTH_RANGE).all()
    else:
        d = -V[..., 2]
        u, v = V[..., 0] / d * (h / 2) + w / 2, h / 2 - V[..., 1] / d * (h / 2)
        assert (d >= 2.0 * NEAR).all() and (d <= 0.5 * RS.FAR).all()
    r, q = np.divmod(idx, cells + 1)
    for on, coord, lo in ((q == 0, u, True), (q == cells, u, False), (r == 0, v, True), (r == cells, v, False)):
        edge = coord[on]
        assert len(edge) and ((edge <= -2.0).all() if lo else (edge >= (w if coord is u else h) + 2.0).all())


@pytest.mark.parametrize("name", NAMES)
def test_closed_sheets_have_no_hole(builds, name):
    """a fold-free sheet that overhangs the picture all round: every centre has a triangle, in the boxed draw as in the brute one; for the
    mesh the triangle is the FP64 twin's or one that shares a vertex with it"""
    target, L = TARGETS[name], builds[name]
    for k, (cells, size) in enumerate(RS.SHEETS):
        if target.name == "shadow":
            size = {(9, 7): (16, 16), (37, 21): (16, 16), (160, 96): (257, 257), (64, 40): (64, 64)}[size]
            if (cells, size) == (64, (16, 16)):
                continue
        P, idx = RS.sheet(target, cells, size, 700 + k)
        V = target.place(P, size)
        sheet_conditions(target, V, idx, cells, size)
        brute = boxed_is_brute(target, L, V, ONE_ORIGIN, size, (0, -1), (name, "sheet", cells, size))
        holes = np.argwhere(brute["words"] == target.empty)
        assert len(holes) == 0, (name, cells, size, holes[:8])
        if target.name != "mesh":
            continue
        assert brute["vertices"]["view_position"].tobytes() == V.reshape(-1, 3).tobytes()
        cam = target.camera(size)
        tw = mesh_twin.draw(brute["vertices"], RS.soup(V)[1], list(cam.position), list(cam.basis), 90.0, size[0], size[1], NEAR, RS.FAR)
        assert tw["hit"].all()
        got = ids_of(brute["words"])
        shared = (idx[got][..., :, None] == idx[tw["tri"]][..., None, :]).any(axis=(-1, -2))
        print(name, cells, size, "the twin's triangle", int((got == tw["tri"]).sum()), "a neighbour", int((shared & (got != tw["tri"])).sum()))
        assert shared.all(), (cells, size, np.argwhere(~shared)[:8])


# ---- 4. the recorded counts ------------------------------------------------------------------------------------------------------------------------

def count_lines(builds):
    lines = []
    for name in NAMES:
        target, L = TARGETS[name], builds[name]
        size = target.odd if name != "shadow" else (64, 64)
        cases = family_cases(target, size, 250, 500) + [c[:4] for c in placed_cases(target, L)] + layout_cases(target) + [tie_case(target), layer_case(target)]
        for what, V, origins, sz in cases:
            b = target.cpu(L, V, origins, sz, 0, brute=True)
            kinds = np.bincount(b["setups"]["kind"][b["setups"]["kind"] >= 0], minlength=4)
            words = b["words"][b["words"] != target.empty]
            # a tie: a written word whose depth half a second covering triangle reaches too is not counted here; what is, is the centres
            # covered more than once
            lines.append("%-7s %-28s %4d x %-4d pairs %5d  culled %5d lane %5d wave %5d  centres covered %8d  words written %6d  covered more than once %8d"
                         % (name, what, sz[0], sz[1], len(b["setups"]), kinds[1], kinds[LANE], kinds[WAVE], int(b["cover"]["covered"].sum()), len(words),
                            int(b["cover"]["covered"].sum()) - len(words)))
    return lines


def test_recorded_counts_are_this_runs(builds):
    """profiles/raster_edges.txt holds the counts the CPU builds produce on the fixed seeds (RASTER_EDGES_WRITE_COUNTS=1 writes them)"""
    lines = count_lines(builds)
    if os.environ.get("RASTER_EDGES_WRITE_COUNTS") == "1":
        text = open(COUNTS).read() if os.path.exists(COUNTS) else ""
        head, _, tail = text.partition("---- counts ----\n")
        rest = tail.partition("---- end of counts ----\n")[2]
        with open(COUNTS, "w") as f:
            f.write(head + "---- counts ----\n" + "\n".join(lines) + "\n---- end of counts ----\n" + rest)
    text = open(COUNTS).read()
    for ln in lines:
        assert ln in text, ln


# ---- 5. on the device ------------------------------------------------------------------------------------------------------------------------------

def device_cases(target, L):
    """every placed, wave-layout, tie, contention and order case and one random soup a family: (name, V, origins, size, lane_boxes)"""
    cases = [(c[0], c[1], c[2], c[3], (c[4],)) for c in placed_cases(target, L)]
    cases += [(what, V, o, size, (0, -1)) for what, V, o, size in layout_cases(target)]
    what, V, o, size = tie_case(target)
    cases.append((what, V, o, size, (0, 64)))
    what, V, o, size = layer_case(target)
    cases.append((what, V, o, size, (0, 64)))
    fams = family_cases(target, target.sizes[-2], 250, 800)
    cases += [(what, V, o, size, (0,)) for what, V, o, size in fams + family_cases(target, target.sizes[-1], 250, 801)]
    cases.append(("a closed sheet", target.place(RS.sheet(target, 33, target.sizes[-2], 750)[0], target.sizes[-2]), ONE_ORIGIN, target.sizes[-2], (0, -1)))
    what, V, o, size = fams[0]
    for order, perm in RS.orders(len(V), 600).items():
        cases.append((what + ", " + order, V[perm], o, size, (0,)))
    return cases


def device_is_brute(target, L, ctx, V, origins, size, lane_box, what):
    brute = target.cpu(L, V, origins, size, lane_box, brute=True)
    got = target.gpu(ctx, V, origins, size, lane_box)
    if got["words"] is not None:
        assert got["words"].tobytes() == brute["words"].tobytes(), (what, "words")
    assert got["drawn"] == brute["drawn"], (what, "lane + wave")
    if target.name == "mesh":
        assert_same_picture(got, target.cpu(L, V, origins, size, lane_box), what)
    if target.name == "solid":
        same_picture(got, brute, what)
        same_picture(got, target.cpu(L, V, origins, size, lane_box), what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_walk_writes_the_brute_passes_words(builds, name):
    """ow_mesh_draw, ow_solid_draw_instances and ow_shadow_map_cast_instances over zero maps: the visibility words and the map byte for
    byte the brute pass's (the solid draw's through its records), lane + wave the same count, and the records and RGBA8 words the boxed
    CPU build's"""
    target, L = TARGETS[name], builds[name]
    ctx = target.context()
    for what, V, origins, size, lane_boxes in device_cases(target, L):
        for lane_box in lane_boxes:
            device_is_brute(target, L, ctx, V, origins, size, lane_box, (name, what, lane_box))
    ctx.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_draw_repeated_three_times_gives_the_same_bytes(builds, name):
    """4 096 layers racing on every word through the unlocked pre-read, and 129 pairs with the wave's in the last lane of a partial wave"""
    target, L = TARGETS[name], builds[name]
    ctx = target.context()
    what, V, o, size = [c for c in layout_cases(target) if c[0].startswith("129")][0]
    for case in (layer_case(target), (what, V, o, size)):
        for lane_box in (0, 64):
            runs = [device_is_brute(target, L, ctx, case[1], case[2], case[3], lane_box, (name, case[0], lane_box, k)) for k in range(3)]
            for r in runs[1:]:
                for key in ("words", "rec", "rgba"):
                    assert (r[key] is None and runs[0][key] is None) or r[key].tobytes() == runs[0][key].tobytes(), (name, case[0], lane_box, key)
    ctx.free()
