"""queue_order 1 -- a pass's camera rays queued cell by cell, all sub-frames of a cell together (strelka_amd/csrc/skh_order.h) -- changes where a ray waits and
nothing else: the accumulated image is byte-identical to queue_order 0's and the same rays are traced, at every cell size, through a custom tile list, an adaptive
render with frozen tiles, and the one-call-per-sub-frame pattern with its look-ahead passes.  200 x 120 at tile 32: partial tiles on two sides, 56 raygen blocks."""
import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes

pytestmark = pytest.mark.gpu

W, H, TILE, DEPTH = 200, 120, 32, 4
CELLS = (-1, 1, 2)  # an eighth of a block (one 64-slot chunk), one block, two (a whole 32 x 32 tile)
SUBSET = [(x, y) for y in range(0, H, TILE) for x in range(0, W, TILE)][::-2]  # every second tile, listed backwards
SCENES = {"cornell": scenes.cornell_box, "kitchen": lambda: scenes.kitchen_standin(seed=7, n_meshes=12, n_instances=60, tri_lo=100, tri_hi=1500)}
_scene_cache = {}


def scene(name):
    if name not in _scene_cache:
        sc = SCENES[name]()
        _scene_cache[name] = (sc, sc.arrays())
    return _scene_cache[name]


def render(name, mode, n, options):
    """One frame of n sub-frames in a fresh context -> (accum, (radiance rays, shadow rays), extra)"""
    from strelka_amd import build, capi

    build.build()
    sc, arr = scene(name)
    ctx = capi.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_scene(arr)
    ctx.set_tiles(TILE, SUBSET if mode == "tiles" else None)
    ctx.resize(W, H)
    cam = sc.getCamera()
    if mode == "adaptive":
        # passes of 2, 3, 3 sub-frames, a check after each.  A tile freezes when the relative standard error of every pixel is at most the threshold: 2 % is out of reach
        # of a path-traced pixel in five samples, and met at once where both samples are equal -- the Cornell box seen from far enough back that the tiles along the
        # border see only void (tests/test_adaptive_cpu.py's view).  The kitchen is a closed room: nothing of it freezes in eight samples at any bar worth the name
        # (measured: none at 25 %), so there the case holds the adaptive passes' own tables with every tile active
        ctx.set_adaptive(threshold=0.02 if name == "cornell" else 0.25, dark_level=0.2, min_samples=2, interval=3)
        if name == "cornell":
            cam = S.Camera(fov=cam.fov)
            cam.lookAt((0.0, 0.0, 7.0), (0.0, 0.0, 0.0))
    ctx.reset_stats()
    exposure = np.full(3, 1.0, np.float32) if mode == "adaptive" else None  # (the checks look at the tone-mapped luminance)
    params = lambda i: S.frame_params(cam, W, H, subframe_index=i, spp_total=n, max_depth=DEPTH, exposure=exposure)
    if mode == "calls":
        for i in range(n):
            ctx.render_subframe(params(i))
    else:
        ctx.render_subframes(params(0), n)
    st = ctx.stats()
    extra = (ctx.adaptive_info(), ctx.read_adaptive()) if mode == "adaptive" else None
    out = (ctx.read_accum(), (st["rays_radiance"], st["rays_shadow"]), extra)
    ctx.close()
    return out


_reference = {}


def reference(name, mode, n):
    """queue_order 0, computed once per case and shared"""
    key = (name, mode, n)
    if key not in _reference:
        _reference[key] = render(name, mode, n, {"queue_order": 0})
    return _reference[key]


def same(got, want):
    assert got[1] == want[1] and got[1][0] > 0 and got[1][1] > 0
    assert got[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("n", (2, 5, 8))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_image_and_the_rays_do_not_depend_on_the_order(name, n, cell):
    same(render(name, "plain", n, {"queue_order": 1, "cell_blocks": cell}), reference(name, "plain", n))


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_through_a_tile_subset(name, cell):
    want = reference(name, "tiles", 5)
    assert 0 < want[1][0] < reference(name, "plain", 5)[1][0]  # (the subset leaves pixels out)
    same(render(name, "tiles", 5, {"queue_order": 1, "cell_blocks": cell}), want)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_through_an_adaptive_render_with_frozen_tiles(name, cell):
    want = reference(name, "adaptive", 8)
    info = want[2][0]
    print(name, info)
    if name == "cornell":  # tiles froze at the first check, others went on to the end: the passes of 3 ran with tiles left out
        assert info["checks"] == 3 and info["min_observations"] == 2 and info["max_observations"] == 8 and 0 < info["active_tiles"] < info["tiles"]
    got = render(name, "adaptive", 8, {"queue_order": 1, "cell_blocks": cell})
    same(got, want)
    assert got[2][0] == info and got[2][1].tobytes() == want[2][1].tobytes()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_one_call_per_subframe_with_look_ahead(name, cell):
    """n calls of render_subframe -- the library traces 2, 4, 8 sub-frames ahead, each pass size with tables of its own -- against one render_subframes(n)"""
    got = render(name, "calls", 8, {"queue_order": 1, "cell_blocks": cell})
    assert got[0].tobytes() == reference(name, "plain", 8)[0].tobytes()
    assert got[1] == reference(name, "calls", 8)[1]


def test_with_the_split_phase_and_chunked_cursors():
    same(render("kitchen", "plain", 5, {"queue_order": 1, "cell_blocks": 1, "tail_split": 2, "fetch_chunk": 7}), reference("kitchen", "plain", 5))
