"""Adaptive sampling on the GPU ("Adaptive sampling"): skh_set_adaptive, the statistics and decision kernels of csrc/skh_adapt.h and the
host loop around them.

The yardsticks are the device's own non-adaptive frame and tests/adaptref.py: per-launch images (accumulation off, one launch per call) give the observations,
snapshots of the non-adaptive accumulator and AOVs after every launch give what a tile frozen after n observations must hold.  Every comparison is array_equal.
The scene and its parameters are those of tests/test_adaptive_cpu.py, where the CPU oracle shows that the schedule has all three kinds of tile.
Every test here fails without the feature: the entry points do not exist."""
import numpy as np
import pytest

from strelka_amd import scene as S
from tests import adaptref, blendref, cutref
from tests.test_adaptive_cpu import (DARK_LEVEL, EXPOSURE, H, INTERVAL, MIN_SAMPLES, PARTIAL_TILE, RECORDED_HIST, SPP, THRESHOLD, TILE, W, adaptive_scene,
                                     params)
from tests.test_gpu_cutout import make_ctx, with_environment

pytestmark = pytest.mark.gpu

RAYS = ("rays_radiance", "rays_shadow")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def nan_image():
    import torch

    return torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")


def new_ctx(load, tile=TILE, tiles=None, **options):
    c = make_ctx(**options)
    load(c)
    c.set_tiles(tile, tiles)
    c.resize(W, H)
    return c


def rays_of(c):
    st = c.stats()
    return tuple(st[k] for k in RAYS)


class Reference:
    """the non-adaptive device frame of a scene: obs[k] the image launch k hands to the accumulator, snaps[n] = (accum, diffuse AOV, specular AOV) after n launches"""

    def __init__(self, sc, load, spl=1):
        self.sc, self.load, self.spl, self.launches = sc, load, spl, SPP // spl
        c = new_ctx(load)
        obs = []
        for k in range(self.launches):
            img = nan_image()
            c.render_subframes(params(sc, k * spl, spl, enable_accumulation=0), 1, img.data_ptr())
            obs.append(img.cpu().numpy()[..., :3].copy())
        self.obs = np.stack(obs)
        assert np.isfinite(self.obs).all()
        c.close()
        c = new_ctx(load)
        c.reset_stats()
        self.snaps, self.rays = {}, {0: (0, 0)}
        for k in range(self.launches):
            c.render_subframes(params(sc, k * spl, spl), 1)
            self.snaps[k + 1] = (c.read_accum(), c.read_aov(0), c.read_aov(1))
            self.rays[k + 1] = rays_of(c)
        c.close()
        self._sched = {}

    def schedule(self, tile=TILE, tiles=None, threshold=THRESHOLD, dark=DARK_LEVEL, min_samples=MIN_SAMPLES, interval=INTERVAL, launches=None):
        key = (tile, None if tiles is None else tuple(map(tuple, tiles)), threshold, dark, min_samples, interval, launches)
        if key not in self._sched:
            self._sched[key] = adaptref.schedule(self.obs[:launches], EXPOSURE, tile, threshold, dark, min_samples, interval, tiles)
        return self._sched[key]

    def check(self, c, tile=TILE, tiles=None, **kw):
        """counts and statistics of context c against adaptref; accumulator and AOVs of every tile against the snapshot at the tile's count"""
        r = self.schedule(tile, tiles, **kw)
        state = c.read_adaptive()
        cm = adaptref.count_map(r, W, H, tile)
        assert np.array_equal(state[..., 0], cm.astype(np.float32)), "per-tile observation counts"
        for j, what in enumerate(("n", "mean", "M2", "q")):
            assert same(state[..., j], r["state"][..., j]), what
        got = (c.read_accum(), c.read_aov(0), c.read_aov(1))
        for (x0, y0), n in zip(r["tiles"], r["counts"]):
            sl = (slice(y0, min(H, y0 + tile)), slice(x0, min(W, x0 + tile)))
            for g, s, what in zip(got, self.snaps[n], ("accumulator", "diffuse AOV", "specular AOV")):
                assert same(g[sl], s[sl]), (what, x0, y0, n)
        info = c.adaptive_info()
        counts = np.array(r["counts"])
        assert info["enabled"] == 1 and info["tiles"] == len(counts) and info["checks"] == r["checks"]
        assert info["min_observations"] == counts.min() and info["max_observations"] == counts.max()
        assert info["active_tiles"] == sum(1 for f in r["frozen"] if not f)
        valid = np.array([(min(H, y0 + tile) - y0) * (min(W, x0 + tile) - x0) for x0, y0 in r["tiles"]])
        assert info["pixel_observations"] == int((valid * counts).sum())
        return r, got, state


def cornell_loader(sc):
    arr = sc.arrays()
    return lambda c: c.set_scene(arr)


@pytest.fixture(scope="module")
def ref():
    sc = adaptive_scene()
    return Reference(sc, cornell_loader(sc))


@pytest.fixture(scope="module")
def ref2():
    sc = adaptive_scene()
    return Reference(sc, cornell_loader(sc), spl=2)


def adaptive_ctx(r, tile=TILE, tiles=None, threshold=THRESHOLD, dark=DARK_LEVEL, min_samples=MIN_SAMPLES, interval=INTERVAL, **options):
    c = new_ctx(r.load, tile, tiles, **options)
    c.set_adaptive(threshold, dark, min_samples, interval)
    c.reset_stats()
    return c


def whole_frame(c, r, how="one"):
    """the frame through one of the entry points: one skh_render_subframes call, one skh_render_subframe call per launch, or chunks of 3 launches"""
    L, spl = r.launches, r.spl
    if how == "one":
        c.render_subframes(params(r.sc, 0, spl), L)
    elif how == "each":
        for k in range(L):
            c.render_subframe(params(r.sc, k * spl, spl))
    else:
        for k in range(0, L, 3):
            c.render_subframes(params(r.sc, k * spl, spl), min(3, L - k))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the schedule and the image
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [TILE, PARTIAL_TILE])
def test_schedule_and_image(ref, tile):
    c = adaptive_ctx(ref, tile)
    whole_frame(c, ref)
    r, _, state = ref.check(c, tile)
    counts = np.array(r["counts"])
    hist = {int(k): int((counts == k).sum()) for k in np.unique(counts)}
    print("tile", tile, "observations -> tiles", hist)
    assert hist == RECORDED_HIST[tile]  # (the device's per-launch images are the CPU oracle's: all three kinds of tile)
    info = c.adaptive_info()
    assert info["active_tiles"] == sum(1 for f in r["frozen"] if not f)
    assert info["pixel_observations"] + info["pixel_observations_saved"] == W * H * SPP
    # only the rays that were traced are counted: fewer than the full frame's
    assert 0 < rays_of(c)[0] < ref.rays[SPP][0]
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: the entry points agree
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spl", [1, 2])
def test_entry_points_agree(ref, ref2, spl):
    r = ref if spl == 1 else ref2
    out = []
    for how in ("one", "each", "chunks"):
        c = adaptive_ctx(r)
        whole_frame(c, r, how)
        _, got, state = r.check(c)
        out.append((got, state, rays_of(c), c.adaptive_info()))
        c.close()
    for got, state, rays, info in out[1:]:
        for a, b in zip(got, out[0][0]):
            assert same(a, b)
        assert same(state, out[0][1]) and rays == out[0][2] and info == out[0][3]
    assert len(np.unique(out[0][1][..., 0])) >= 3  # (the schedule of this launch size is not vacuous either)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: off is off
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(ref):
    full, full_rays = ref.snaps[SPP], ref.rays[SPP]
    # min_samples = spp_total: nothing can stop before the end
    c = adaptive_ctx(ref, threshold=1e3, min_samples=SPP)
    whole_frame(c, ref)
    for a, b in zip((c.read_accum(), c.read_aov(0), c.read_aov(1)), full):
        assert same(a, b)
    assert rays_of(c) == full_rays and (c.read_adaptive()[..., 0] == SPP).all()
    # ... and after skh_set_adaptive(NULL) the context is the one that never heard of the feature
    c.set_adaptive(None)
    assert c.adaptive_info()["enabled"] == 0 and (c.read_adaptive() == 0).all()
    c.reset_stats()
    whole_frame(c, ref, "chunks")
    assert same(c.read_accum(), full[0]) and rays_of(c) == full_rays
    c.close()
    # debug views and frames without accumulation ignore a setting that would stop everything at the first check
    plain, c = new_ctx(ref.load), adaptive_ctx(ref, threshold=1e3)
    plain.reset_stats()
    for kw in ({"debug": 2}, {"enable_accumulation": 0}):
        imgs = []
        for x in (plain, c):
            img = nan_image()
            x.render_subframes(params(ref.sc, 0, **kw), 8, img.data_ptr())
            imgs.append(img.cpu().numpy())
        assert same(imgs[0], imgs[1]) and np.isfinite(imgs[0]).all()
        assert rays_of(plain) == rays_of(c) and c.adaptive_info()["checks"] == 0 and (c.read_adaptive() == 0).all()
    plain.close(), c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: d_image is whole
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_d_image_is_whole(ref):
    c = adaptive_ctx(ref)
    for k in range(0, SPP, 3):  # a fresh buffer every call
        img = nan_image()
        c.render_subframes(params(ref.sc, k), min(3, SPP - k), img.data_ptr())
        got = img.cpu().numpy()
        assert np.isfinite(got).all() and same(got, c.read_accum()), k
    ref.check(c)
    c.close()
    # every tile frozen at the first check: the call after it traces nothing and still writes the whole image
    c = adaptive_ctx(ref, threshold=1e3)
    c.render_subframes(params(ref.sc, 0), 6)
    info, rays = c.adaptive_info(), rays_of(c)
    assert info["active_tiles"] == 0 and info["checks"] == 1 and rays == ref.rays[MIN_SAMPLES] and (c.read_adaptive()[..., 0] == MIN_SAMPLES).all()
    for entry in (c.render_subframe, lambda p, d: c.render_subframes(p, 5, d)):
        img = nan_image()
        entry(params(ref.sc, 6), img.data_ptr())
        assert same(img.cpu().numpy(), ref.snaps[MIN_SAMPLES][0]) and rays_of(c) == rays
    assert same(c.read_accum(), ref.snaps[MIN_SAMPLES][0])
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: ownership
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_tiles_dealt_to_two_contexts(ref):
    grid = adaptref.tile_grid(W, H, TILE)
    whole = ref.schedule()
    deal = [[t for k, t in enumerate(grid) if (k * 7 // 3) % 2 == who] for who in (0, 1)]
    assert len(deal[0]) > 8 and len(deal[1]) > 8
    for mine in deal:
        c = adaptive_ctx(ref, tiles=np.array(mine, np.uint32))
        whole_frame(c, ref)
        r, got, state = ref.check(c, tiles=mine)
        own = np.zeros((H, W), bool)
        for x0, y0 in mine:
            own[y0:y0 + TILE, x0:x0 + TILE] = True
            assert r["counts"][r["tiles"].index((x0, y0))] == whole["counts"][whole["tiles"].index((x0, y0))]
        assert same(state[own], whole["state"][own]) and (state[~own] == 0).all()
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: restart
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_restart_and_thaw(ref):
    c = adaptive_ctx(ref)
    whole_frame(c, ref)
    first = c.adaptive_info()
    assert first["active_tiles"] < first["tiles"]
    # sub-frame 0 begins a frame: every tile is rendered again
    c.reset_stats()
    c.render_subframes(params(ref.sc, 0), 2)
    info = c.adaptive_info()
    assert info["active_tiles"] == info["tiles"] and info["checks"] == 0 and (c.read_adaptive()[..., 0] == 2).all() and same(c.read_accum(), ref.snaps[2][0])
    c.render_subframes(params(ref.sc, 2), SPP - 2)
    ref.check(c)
    assert c.adaptive_info() == first
    # a scene setter in mid-frame thaws everything and clears the statistics
    c.render_subframes(params(ref.sc, 0), 9)
    assert c.adaptive_info()["active_tiles"] < first["tiles"]
    c.set_lights(ref.sc.arrays()["lights"])
    assert c.adaptive_info()["active_tiles"] == first["tiles"]
    img = nan_image()
    c.render_subframes(params(ref.sc, 9), 3, img.data_ptr())
    info = c.adaptive_info()
    assert info["active_tiles"] == info["tiles"] and info["checks"] == 0 and (c.read_adaptive()[..., 0] == 3).all() and np.isfinite(img.cpu().numpy()).all()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: the stages that read the tile list for a path's identity
# ---------------------------------------------------------------------------------------------------------------------------------------------
MIXED_THRESHOLD = 0.12


def mixed_scene():
    """a card with a cutout above a card with a blend material (opacity 0.5), under an environment and a rect light"""
    layers = cutref.CARD_XFORMS["layers"]

    def more(sc):
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
        assert mat == 2
        sc.createInstance(S.INSTANCE_MESH, cutref.card_mesh(sc), mat, layers[0])
        with_environment(sc)

    sc, cut, _ = cutref.card_scene(False, "layers", xforms=[layers[2]], extra=more)
    arr = sc.arrays()

    def load(c):
        c.set_scene(arr)
        c.set_material_cutouts(cut)
        c.set_material_blend(blendref.table(3, {2: blendref.constant(0.5)}))

    return sc, load


def test_mixed_scene():
    sc, load = mixed_scene()
    r = Reference(sc, load)
    c = adaptive_ctx(r, threshold=MIXED_THRESHOLD)
    whole_frame(c, r)
    assert c.cutout_info()["continued_closest"] > 0 and c.blend_info()["passed_radiance"] > 0
    res, _, _ = r.check(c, threshold=MIXED_THRESHOLD)
    counts = np.array(res["counts"])
    print("mixed scene: observations -> tiles", {int(k): int((counts == k).sum()) for k in np.unique(counts)})
    assert (counts < SPP).any() and (counts > MIN_SAMPLES).any()
    c.close()
    c = adaptive_ctx(r, threshold=MIXED_THRESHOLD)
    whole_frame(c, r, "chunks")
    r.check(c, threshold=MIXED_THRESHOLD)
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9: the host adapter: HipRender::setAdaptiveSampling / isConverged in hdRunner's frame loop
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_adapter_converges(tmp_path):
    from tests.test_host_cpp import run_host

    out = run_host(tmp_path, "gpu-adaptive", 6)  # (host_test.cpp: refused parameters, converged after the first check, a stable image and no rays after it, off again)
    assert "host_test gpu-adaptive ok: subframeIndex 5" in out
