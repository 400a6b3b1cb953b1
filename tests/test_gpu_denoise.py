"""The denoiser on the device (skh_denoise; DESIGN.md section 2, "Denoiser") against its definition in float64 (tests/denoiseref.py) under that file's
written-out error bar.  No pixel is excluded from any comparison: the definition has no discontinuity.  Every test calls the new entry point, so each fails
without the feature.

Synthetic planes (denoiseref.synthetic, 67 x 45: a multiple of no workgroup shape, and at step 32 most taps leave it) go to the device through skh_buffer_upload.
Figures on an MI355X (worst error / bar): docs/LOG.md has the table the tests print."""
import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import denoiseref as R

pytestmark = pytest.mark.gpu

INF = float("inf")
NAMES = ("color", "ids", "normal", "position", "albedo")


class Device:
    """a context and device copies of one set of planes"""

    def __init__(self, ctx, planes):
        self.ctx, self.planes = ctx, planes
        self.h, self.w = planes["ids"].shape[:2]
        self.bytes = 16 * self.w * self.h
        self.d = {n: ctx.buffer_alloc(self.bytes) for n in NAMES + ("out",)}
        for n in NAMES:
            ctx.buffer_upload(self.d[n], planes[n])

    def set_color(self, color):
        self.ctx.buffer_upload(self.d["color"], np.ascontiguousarray(color, np.float32))

    def download(self, name="out"):
        out = np.zeros((self.h, self.w, 4), np.float32)
        self.ctx.buffer_download(self.d[name], out)
        return out

    def run(self, p, in_place=False, albedo=True):
        d = self.d
        self.ctx.denoise_device(p, d["color"], d["ids"], d["normal"], d["position"], d["albedo"] if albedo else None, d["color"] if in_place else d["out"])
        return self.download("color" if in_place else "out")

    def ref(self, p, color=None):
        s = self.planes
        return R.denoise(s["color"] if color is None else color, s["ids"], s["normal"], s["position"], s["albedo"], p)

    def free(self):
        for v in self.d.values():
            self.ctx.buffer_free(v)


@pytest.fixture(scope="module")
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx, R.synthetic())
    yield d
    d.free()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. each level alone against float64
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 3, 1, 2])
@pytest.mark.parametrize("lvl", range(7))
def test_each_level_alone_against_float64(dev, lvl, flags):
    p = R.params(dev.w, dev.h, first_level=lvl, levels=1, flags=flags)
    got, ref = dev.run(p), dev.ref(p)
    ratio = R.check(got, dev.planes["color"], ref)
    print(f"level {lvl} flags {flags}: worst error / bar {ratio:.3f} over {int(ref['surface'].sum())} surface pixels of {dev.w * dev.h}, none excluded; widest bar {ref['bar'].max():.2e}")
    assert ratio <= 1.0
    assert not np.array_equal(got[ref["surface"]], dev.planes["color"][ref["surface"]])  # (it filtered)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. bits: one call of five levels == five chained calls == in place == again
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_levels_in_one_call_equal_chained_calls_bit_for_bit(dev):
    p5 = R.params(dev.w, dev.h, levels=5, flags=3)
    whole = dev.run(p5)
    again = dev.run(p5)
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))  # a second identical call
    try:
        for lvl in range(5):
            p1 = R.params(dev.w, dev.h, first_level=lvl, levels=1, flags=(1 if lvl == 0 else 0) | (2 if lvl == 4 else 0))
            step = dev.run(p1, in_place=True)  # (the colour buffer carries the chain)
        assert np.array_equal(step.view(np.uint32), whole.view(np.uint32))
    finally:
        dev.set_color(dev.planes["color"])
    in_place = dev.run(p5, in_place=True)
    dev.set_color(dev.planes["color"])
    assert np.array_equal(in_place.view(np.uint32), whole.view(np.uint32))
    # ... and the five levels are inside the chained bar of the float64 reference
    ratio = R.check(whole, dev.planes["color"], dev.ref(p5))
    print(f"levels 0-4, both flags: worst error / bar {ratio:.3f}")
    assert ratio <= 1.0
    # no flag: the albedo plane may be NULL
    p0 = R.params(dev.w, dev.h, levels=2, flags=0)
    assert np.array_equal(dev.run(p0, albedo=False).view(np.uint32), dev.run(p0).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. pass-through
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pass_through(dev):
    s = dev.planes
    p = R.params(dev.w, dev.h, levels=5, flags=3)
    got = dev.run(p)
    kind = s["ids"][..., 3]
    other = (kind == 0) | (kind == 3) | ~np.isfinite(s["color"][..., :3]).all(axis=-1)
    assert other.sum() == 42 + 42 + 2
    assert np.array_equal(got[other].view(np.uint32), s["color"][other].view(np.uint32))
    assert np.array_equal(got[..., 3].view(np.uint32), s["color"][..., 3].view(np.uint32))  # every alpha word, the NaN patterns among them
    assert np.array_equal(~np.isfinite(got[..., :3]), ~np.isfinite(s["color"][..., :3]))  # no non-finite value where the input had none
    assert not np.array_equal(got[5, 8, :3], s["color"][5, 8, :3]) and not np.array_equal(got[35, 51, :3], s["color"][35, 51, :3])  # (their neighbours were filtered)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. image borders and the grid's last partial workgroup
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63)])
def test_shapes_against_float64(ctx, w, h):
    d = Device(ctx, R.synthetic(w, h, seed=w + h, special=False))
    try:
        for first, levels in ((0, 3), (5, 1)):
            p = R.params(w, h, first_level=first, levels=levels, flags=3)
            ratio = R.check(d.run(p), d.planes["color"], d.ref(p))
            print(f"{w} x {h}, levels {first}..{first + levels - 1}: worst error / bar {ratio:.3f}")
            assert ratio <= 1.0
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. closed forms on the device
# ---------------------------------------------------------------------------------------------------------------------------------------------
def spline_kernel(levels):
    """the 1-D response of `levels` a-trous levels of h: h convolved with itself at steps 1, 2, 4, ..."""
    k = np.ones(1)
    for lvl in range(levels):
        up = np.zeros(4 * (1 << lvl) + 1)
        up[:: 1 << lvl] = R.H5
        k = np.convolve(k, up)
    return k


def test_constant_colour_and_the_impulse_response(ctx):
    n = 33
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    planes = {k: np.zeros((n, n, 4), np.uint32 if k == "ids" else np.float32) for k in NAMES}
    planes["ids"][..., 3] = 1
    planes["normal"][..., 2], planes["position"][..., 0], planes["position"][..., 1] = 1.0, x * 0.1, y * 0.1
    planes["albedo"][...] = 1.0
    planes["color"][..., :3], planes["color"][..., 3] = [0.3, 1.7, 1e-3], 1.0
    d = Device(ctx, planes)
    try:
        # a constant colour comes back, within the bar (K u |c|: every weight error cancels)
        p = R.params(n, n, levels=3, flags=0)
        got, ref = d.run(p), d.ref(p)
        assert R.check(got, planes["color"], ref) <= 1.0 and np.abs(ref["out"] - planes["color"][..., :3]).max() < 1e-15
        assert np.abs(got[..., :3] - planes["color"][..., :3]).max() <= 3 * 51 * R.U * 1.7
        # one bright pixel, sigma_color = +inf, two levels: the tensor product of the B3 spline cascade (support 13, inside the image for the centre)
        imp = np.zeros((n, n, 4), np.float32)
        imp[n // 2, n // 2, :3] = [1.0, 2.0, 0.5]
        d.set_color(imp)
        p = R.params(n, n, levels=2, flags=0, sigma_color=INF)
        got, ref = d.run(p), d.ref(p, color=imp)
        k = spline_kernel(2)
        assert len(k) == 13 and abs(k.sum() - 1.0) < 1e-15
        want = np.zeros((n, n))
        want[n // 2 - 6:n // 2 + 7, n // 2 - 6:n // 2 + 7] = np.outer(k, k)
        assert np.abs(ref["out"] - want[..., None] * [1.0, 2.0, 0.5]).max() < 1e-15  # the reference is the closed form ...
        assert R.check(got, imp, ref) <= 1.0  # ... and the device is within the bar of it
        assert (got[..., 0] != 0).sum() == 169 and abs(float(got[..., 0].astype(np.float64).sum()) - 1.0) < 1e-5
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. end to end on the Cornell box
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cornell_box_end_to_end():
    from strelka_amd import capi

    W, H, SPP = 96, 72, 4
    sc = scenes.cornell_box()
    arr, cam = sc.arrays(), sc.getCamera()

    def frames(c, first, count, spp_total, d_image=None):
        for i in range(first, first + count):
            c.render_subframe(S.frame_params(cam, W, H, subframe_index=i, spp_total=spp_total, max_depth=4), d_image)

    a, b, truth = capi.Context(0), capi.Context(0), capi.Context(0)
    try:
        for c in (a, b, truth):
            c.set_scene(arr)
            c.resize(W, H)
        d_image, d_out = a.buffer_alloc(16 * W * H), a.buffer_alloc(16 * W * H)
        frames(a, 0, SPP, 64, d_image)
        frames(b, 0, SPP, 64)
        noisy = np.zeros((H, W, 4), np.float32)
        a.buffer_download(d_image, noisy)
        guides = a.render_guides(S.aov_params(cam, W, H))
        assert set(guides) == set(capi.DENOISE_GUIDES) and a.aov_info()["calls"] == 1
        accum_before, stats_before = a.read_accum(), a.stats()
        p = S.denoise_params(W, H, scene=arr, image=noisy, guides=guides)  # the defaults
        assert capi.denoise_check(p) and int(p["levels"]) == 5 and int(p["flags"]) == 3
        # the device path on the image the renderer wrote, and the numpy path on its download: the same bits
        bufs = {n: a.buffer_alloc(16 * W * H) for n in capi.DENOISE_GUIDES}
        for n, buf in bufs.items():
            a.buffer_upload(buf, guides[n])
        a.denoise_device(p, d_image, bufs["ids"], bufs["normal"], bufs["position"], bufs["albedo"], d_out)
        got = np.zeros((H, W, 4), np.float32)
        a.buffer_download(d_out, got)
        assert np.array_equal(got.view(np.uint32), a.denoise(noisy, guides, p).view(np.uint32))
        # the glue: the reference applied to the downloaded planes
        ref = R.denoise(noisy, guides["ids"], guides["normal"], guides["position"], guides["albedo"], p)
        ratio = R.check(got, noisy, ref)
        print(f"cornell box {W} x {H}, {SPP} spp, five levels: worst error / bar {ratio:.3f} over {int(ref['surface'].sum())} surface pixels; sigma_color {float(p['sigma_color']):.4f}, "
              f"sigma_plane {float(p['sigma_plane']):.4f}")
        assert ratio <= 1.0 and ref["surface"].sum() > 0.5 * W * H  # (the box fills two thirds of the frame)
        # nothing of the frame moved
        stats_after = a.stats()
        assert np.array_equal(a.read_accum().view(np.uint32), accum_before.view(np.uint32))
        assert (stats_after["rays_radiance"], stats_after["rays_shadow"]) == (stats_before["rays_radiance"], stats_before["rays_shadow"])
        frames(a, SPP, 1, 64)
        frames(b, SPP, 1, 64)
        assert np.array_equal(a.read_accum().view(np.uint32), b.read_accum().view(np.uint32))  # the next sub-frame, against a context that never denoised
        info = a.denoise_info()
        assert info["calls"] == 2 and info["pixels"] == 2 * W * H and info["scratch_bytes"] >= 56 * W * H and b.denoise_info()["scratch_bytes"] == 0
        # closer to the converged frame than the input was
        truth.render_subframes(S.frame_params(cam, W, H, subframe_index=0, spp_total=1024, max_depth=4), 1024)
        want = truth.read_accum()[..., :3].astype(np.float64)
        surf = ref["surface"]
        rms = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - want)[surf] ** 2).mean()))
        before, after = rms(noisy), rms(got)
        print(f"rms error against 1024 spp over the surface pixels: {before:.5f} at {SPP} spp, {after:.5f} filtered: ratio {after / before:.3f}")
        assert after < before
        for buf in list(bufs.values()) + [d_image, d_out]:
            a.buffer_free(buf)
    finally:
        for c in (a, b, truth):
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. refusals, and the scratch
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_null_frees_the_scratch(ctx, dev):
    from strelka_amd import capi

    d = dev.d
    sentinel = np.full((dev.h, dev.w, 4), 7.25, np.float32)
    ctx.buffer_upload(d["out"], sentinel)
    good = R.params(dev.w, dev.h, levels=2, flags=3)
    bad = np.array(good)
    bad["levels"] = 9
    zero = np.array(good)
    zero["sigma_normal"] = 0.0
    cases = {"levels 9": (bad, d["color"], d["ids"], d["normal"], d["position"], d["albedo"], d["out"]),
             "sigma 0": (zero, d["color"], d["ids"], d["normal"], d["position"], d["albedo"], d["out"]),
             "no colour": (good, None, d["ids"], d["normal"], d["position"], d["albedo"], d["out"]),
             "no ids": (good, d["color"], None, d["normal"], d["position"], d["albedo"], d["out"]),
             "no normal": (good, d["color"], d["ids"], None, d["position"], d["albedo"], d["out"]),
             "no position": (good, d["color"], d["ids"], d["normal"], None, d["albedo"], d["out"]),
             "no albedo under a flag": (good, d["color"], d["ids"], d["normal"], d["position"], None, d["out"]),
             "no output": (good, d["color"], d["ids"], d["normal"], d["position"], d["albedo"], None)}
    dev.run(good)  # (so that there is a previous state: scratch and counters)
    ctx.buffer_upload(d["out"], sentinel)
    before = ctx.denoise_info()
    for name, args in cases.items():
        with pytest.raises(capi.SkhError, match="skh_denoise"):
            ctx.denoise_device(*args)
        assert np.array_equal(dev.download(), sentinel), name
    after = ctx.denoise_info()
    assert (after["calls"], after["pixels"], after["scratch_bytes"]) == (before["calls"], before["pixels"], before["scratch_bytes"])
    assert before["scratch_bytes"] >= 56 * dev.w * dev.h and before["ms_last"] > 0.0
    # NULL parameters free the scratch; the next call takes it again and gives the same bits
    first = dev.run(good)
    ctx.denoise_device(None, None, None, None, None, None, None)
    assert ctx.denoise_info()["scratch_bytes"] == 0
    assert np.array_equal(dev.run(good).view(np.uint32), first.view(np.uint32)) and ctx.denoise_info()["scratch_bytes"] >= 56 * dev.w * dev.h
    # a larger image regrows it
    big = Device(ctx, R.synthetic(200, 150, special=False))
    try:
        pb = R.params(200, 150, levels=2, flags=3)
        assert R.check(big.run(pb), big.planes["color"], big.ref(pb)) <= 1.0 and ctx.denoise_info()["scratch_bytes"] >= 56 * 200 * 150
    finally:
        big.free()
