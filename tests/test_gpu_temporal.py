"""Temporal accumulation on the device (skh_temporal; DESIGN.md section 2, "Temporal accumulation").  The definition has no transcendental, so the device must
give the bits of its float32 restatement (tests/temporalref.py: reproject32) on every pixel of all three outputs; the float64 reference with its written-out
error bar (reproject64) is the second, independent yardstick on the pixels no decision of which lies inside its rounding error.  Every test calls the new entry
point, so each fails without the feature.

Figures on an MI355X: docs/LOG.md has the lines the tests print."""
import copy
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import temporalref as R

pytestmark = pytest.mark.gpu

CURRENT = ("color", "ids", "normal", "position", "albedo")
PREVIOUS = ("history", "ids", "normal", "position")
OUTPUTS = ("image", "history", "motion")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Device:
    """a context and device copies of one synthetic input (temporalref.synthetic's dictionary)"""

    def __init__(self, ctx, s):
        self.ctx, self.s = ctx, s
        self.h, self.w = s["ids"].shape[:2]
        nbytes = 16 * self.w * self.h
        self.d = {n: ctx.buffer_alloc(nbytes) for n in CURRENT + tuple("prev_" + n for n in PREVIOUS) + OUTPUTS}
        for n in CURRENT:
            ctx.buffer_upload(self.d[n], s[n])
        for n in PREVIOUS:
            ctx.buffer_upload(self.d["prev_" + n], s["prev"][n])

    def fill(self, name, value):
        self.ctx.buffer_upload(self.d[name], np.full((self.h, self.w, 4), value, np.float32))

    def download(self, name):
        out = np.zeros((self.h, self.w, 4), np.float32)
        self.ctx.buffer_download(self.d[name], out)
        return out

    def args(self, p, prev=True, motion=True, out="image", albedo=True):
        d = self.d
        return [p, d["color"], d["ids"], d["normal"], d["position"], d["albedo"] if albedo else None] + [d["prev_" + n] if prev else None for n in PREVIOUS] + [
            d[out], d["history"], d["motion"] if motion else None]

    def run(self, p, **kw):
        self.ctx.temporal_device(*self.args(p, **kw))
        return {n: self.download(n) for n in OUTPUTS}

    def refs(self, p, prev=True):
        s = self.s
        a = (s["color"], s["ids"], s["normal"], s["position"], s["albedo"], s["prev"] if prev else None, p)
        return R.reproject32(*a), R.reproject64(*a)

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


def with_flags(p, flags):
    q = np.array(p)
    q["flags"] = flags
    return q


def compare(d, p, prev, label):
    """the device against both references: every pixel of the three outputs bit for bit against float32, the unambiguous ones inside float64's bar"""
    got = d.run(p, prev=prev)
    want, ref = d.refs(p, prev=prev)
    differing = {n: int((bits(got[n]) != bits(want[n])).any(axis=-1).sum()) for n in OUTPUTS}
    ratio = R.check(got, d.s["color"], ref)
    surf = ref["surface"]
    print(f"{label}: pixels that differ from the float32 restatement {differing} of {d.w * d.h}; worst error / float64 bar {ratio:.3f} over "
          f"{int((surf & ~ref['ambiguous']).sum())} unambiguous of {int(surf.sum())} surface pixels")
    for n in OUTPUTS:
        assert np.array_equal(bits(got[n]), bits(want[n])), (label, n)
    assert ratio <= 1.0
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the bits, and the bar
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("flags", [R.DEMODULATE, 0])
def test_synthetic_bit_for_bit_and_inside_the_bar(dev, flags, prev):
    p = with_flags(dev.s["params"], flags)
    got, ref = compare(dev, p, prev, f"67 x 45, flags {flags}, {'a' if prev else 'no'} previous frame")
    surf = ref["surface"]
    if prev:
        assert (ref["accepted"][surf] == 4).mean() >= 0.5 and (ref["accepted"][surf] == 0).mean() >= 0.05  # (the input exercises every branch)
        assert not np.array_equal(got["image"][surf], dev.s["color"][surf])  # (it blended)
    else:
        assert np.array_equal(got["history"][surf][:, 3], np.full(int(surf.sum()), 1.0, np.float32)) and not got["motion"].any()
        seeded = np.array(p)
        seeded["initial_length"], seeded["max_history"] = 7.0, 8.0
        assert (dev.run(seeded, prev=False)["history"][surf][:, 3] == 7.0).all()  # how a host seeds a history of a known length


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63)])
def test_shapes_bit_for_bit(ctx, w, h):
    """the image borders and the partial 64 x 4 workgroups"""
    d = Device(ctx, R.synthetic(w, h, seed=w + h))
    try:
        for prev in (True, False):
            compare(d, d.s["params"], prev, f"{w} x {h}, {'a' if prev else 'no'} previous frame")
    finally:
        d.free()


def test_in_place_and_without_the_motion_plane(dev):
    p = dev.s["params"]
    whole = dev.run(p)
    # no motion plane: the other two outputs keep their bits, the motion buffer is not written
    dev.fill("motion", 7.25)
    dev.fill("image", 0.0), dev.fill("history", 0.0)
    dev.ctx.temporal_device(*dev.args(p, motion=False))
    assert np.array_equal(bits(dev.download("image")), bits(whole["image"])) and np.array_equal(bits(dev.download("history")), bits(whole["history"]))
    assert (dev.download("motion") == 7.25).all()
    # without DEMODULATE the albedo plane may be NULL
    q = with_flags(p, 0)
    a = dev.run(q)
    dev.ctx.temporal_device(*dev.args(q, albedo=False))
    assert np.array_equal(bits(dev.download("image")), bits(a["image"]))
    # d_out == d_color
    try:
        dev.ctx.temporal_device(*dev.args(p, out="color"))
        assert np.array_equal(bits(dev.download("color")), bits(whole["image"]))
        assert np.array_equal(bits(dev.download("history")), bits(whole["history"])) and np.array_equal(bits(dev.download("motion")), bits(whole["motion"]))
    finally:
        dev.ctx.buffer_upload(dev.d["color"], dev.s["color"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, dev):
    from strelka_amd import capi

    good = np.array(dev.s["params"])

    def edited(**kw):
        q = np.array(good)
        for k, v in kw.items():
            if k == "matrix":
                q["prev_world_to_clip"][5] = v
            elif k == "reserved":
                q["reserved"][v] = 1
            else:
                q[k] = v
        return q

    records = {"zero width": edited(width=0), "zero height": edited(height=0), "more than 2^26 pixels": edited(width=(1 << 13) + 1, height=1 << 13),
               "a NaN matrix entry": edited(matrix=np.nan), "an infinite matrix entry": edited(matrix=np.inf), "normal_min 1.5": edited(normal_min=1.5),
               "normal_min -1.5": edited(normal_min=-1.5), "normal_min nan": edited(normal_min=np.nan), "plane_tolerance 0": edited(plane_tolerance=0.0),
               "plane_tolerance < 0": edited(plane_tolerance=-1.0), "plane_tolerance nan": edited(plane_tolerance=np.nan), "max_history 0.5": edited(max_history=0.5),
               "max_history inf": edited(max_history=np.inf), "max_history nan": edited(max_history=np.nan), "initial_length 0.5": edited(initial_length=0.5),
               "initial_length above max_history": edited(initial_length=33.0), "initial_length nan": edited(initial_length=np.nan),
               "albedo_floor 0": edited(albedo_floor=0.0), "albedo_floor inf": edited(albedo_floor=np.inf), "flag bit 1": edited(flags=3),
               "reserved[0]": edited(reserved=0), "reserved[7]": edited(reserved=7)}
    cases = {name: dev.args(q) for name, q in records.items()}
    for k, name in ((1, "no colour"), (2, "no ids"), (3, "no normal"), (4, "no position"), (5, "no albedo under DEMODULATE"), (7, "a history without its ids"),
                    (8, "a history without its normals"), (9, "a history without its positions"), (10, "no output"), (11, "no history output")):
        a = dev.args(good)
        a[k] = None
        cases[name] = a
    alias = dev.args(good)
    alias[11] = alias[6]  # d_history_out == d_prev_history
    cases["the history written over the one the taps read"] = alias
    dev.run(good)  # (so that there is a previous state: the counters)
    for n in OUTPUTS:
        dev.fill(n, 7.25)
    before = ctx.temporal_info()
    try:
        for name, a in cases.items():
            assert not capi.temporal_check(a[0]) or name not in records, name
            with pytest.raises(capi.SkhError, match="skh_temporal"):
                ctx.temporal_device(*a)
            for n in OUTPUTS:
                assert (dev.download(n) == 7.25).all(), (name, n)
            assert np.array_equal(bits(dev.download("prev_history")), bits(dev.s["prev"]["history"])), name
    finally:
        ctx.buffer_upload(dev.d["prev_history"], dev.s["prev"]["history"])
    after = ctx.temporal_info()
    assert (after["calls"], after["pixels"]) == (before["calls"], before["pixels"]) and before["calls"] >= 1 and before["ms_last"] > 0.0
    assert len(cases) == len(records) + 11


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. a real scene
# ---------------------------------------------------------------------------------------------------------------------------------------------
def orbit(cam0, degrees):
    """the camera turned about the point 3 units ahead of it (bench.py's interactive orbit)"""
    cam = copy.deepcopy(cam0)
    eye0 = np.array(cam.position, np.float64)
    target = eye0 - np.array(cam.rotation[2, :3], np.float64) * 3.0
    a, r = math.radians(degrees), eye0 - target
    cam.lookAt(tuple(target + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])), tuple(target))
    return cam


def sample_frame(c, cam, W, H, index, d_image):
    """one raw sample of the sequence as an image: the call HipRender makes for a moving camera with temporal accumulation on"""
    c.render_subframe(S.frame_params(cam, W, H, subframe_index=index, spp_total=64, max_depth=4, enable_accumulation=0), d_image)
    out = np.zeros((H, W, 4), np.float32)
    c.buffer_download(d_image, out)
    return out


def test_cornell_box_motion_disocclusion_and_an_untouched_frame():
    from strelka_amd import capi

    W, H = 96, 64
    sc = scenes.cornell_box()
    arr = sc.arrays()
    cams = [orbit(sc.getCamera(), 0.0), orbit(sc.getCamera(), 6.0)]
    a, b = capi.Context(0), capi.Context(0)
    try:
        for c in (a, b):
            c.set_scene(arr)
            c.resize(W, H)
        d_image = a.buffer_alloc(16 * W * H)
        aovs = [S.aov_params(cam, W, H) for cam in cams]
        guides = [a.render_guides(q) for q in aovs]
        frames = [sample_frame(a, cams[k], W, H, k, d_image) for k in range(2)]
        # an accumulation in progress, beside a context that never hears of the feature
        for c in (a, b):
            for i in range(3):
                c.render_subframe(S.frame_params(cams[1], W, H, subframe_index=i, spp_total=64, max_depth=4))
        accum, stats, adaptive = a.read_accum(), a.stats(), a.adaptive_info()
        p0 = S.temporal_params(W, H, scene=arr)
        first = a.temporal(frames[0], guides[0], None, p0)
        p1 = S.temporal_params(W, H, aovs[0], scene=arr)
        prev = {"history": first["history"], "ids": guides[0]["ids"], "normal": guides[0]["normal"], "position": guides[0]["position"]}
        got = a.temporal(frames[1], guides[1], prev, p1)
        want = R.reproject32(frames[1], guides[1]["ids"], guides[1]["normal"], guides[1]["position"], guides[1]["albedo"], prev, p1)
        for n in OUTPUTS:
            assert np.array_equal(bits(got[n]), bits(want[n])), n
        # the frame did not move
        after = a.stats()
        assert np.array_equal(bits(a.read_accum()), bits(accum)) and a.adaptive_info() == adaptive
        assert all(after[k] == stats[k] for k in after if k.startswith("rays_")) and after["speculated_discarded"] == stats["speculated_discarded"]
        for c in (a, b):
            c.render_subframe(S.frame_params(cams[1], W, H, subframe_index=3, spp_total=64, max_depth=4))
        assert np.array_equal(bits(a.read_accum()), bits(b.read_accum()))
        info = a.temporal_info()
        assert info["calls"] == 2 and info["pixels"] == 2 * W * H and info["ms_last"] > 0.0 and b.temporal_info()["calls"] == 0
        # the motion plane against the float64 projection of the POSITION plane
        kind = guides[1]["ids"][..., 3]
        surf = ((kind == 1) | (kind == 2)) & np.isfinite(frames[1][..., :3]).all(-1)
        M = np.asarray(aovs[0]["world_to_clip"], np.float64).reshape(4, 4)
        P = np.concatenate([guides[1]["position"][..., :3].astype(np.float64), np.ones((H, W, 1))], -1)
        clip = P @ M.T
        with np.errstate(all="ignore"):
            fx, fy = (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W - 0.5, (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H - 0.5
        yy, xx = np.mgrid[0:H, 0:W]
        inside = surf & (clip[..., 3] > 0) & (fx > -0.99) & (fx < W - 0.01) & (fy > -0.99) & (fy < H - 0.01)
        clear = inside & (np.abs(fx - np.round(fx)) > 1e-3) & (np.abs(fy - np.round(fy)) > 1e-3)  # (not within a float32 rounding of a pixel boundary)
        mv = got["motion"].astype(np.float64)
        assert clear.sum() > 0.5 * W * H
        assert np.abs(mv[..., 0] - (fx - xx))[inside].max() < 1e-3 and np.abs(mv[..., 1] - (fy - yy))[inside].max() < 1e-3
        assert np.array_equal(np.floor(mv[..., 0] + xx)[clear], np.floor(fx)[clear]) and np.array_equal(np.floor(mv[..., 1] + yy)[clear], np.floor(fy)[clear])
        moved = np.hypot(mv[..., 0], mv[..., 1])[inside]
        assert moved.max() > 2.0  # (six degrees at this size: several pixels)
        # disocclusion: a point that was hidden a frame ago -- all four of its taps saw something at least 0.3 units nearer to the previous eye, the far side of a
        # block's silhouette -- has no history.  (The blocks and the room's shell are ONE instance here: the plane and normal tests alone tell them apart.)
        ix, iy = np.floor(np.where(clear, fx, 0)).astype(int), np.floor(np.where(clear, fy, 0)).astype(int)
        eye = np.asarray(cams[0].position, np.float64)
        far = np.linalg.norm(P[..., :3] - eye, axis=-1)
        other = clear.copy()
        for dx, dy in R.TAPS:
            qx, qy = np.clip(ix + dx, 0, W - 1), np.clip(iy + dy, 0, H - 1)
            seen = guides[0]["position"][qy, qx, :3].astype(np.float64)
            other &= (guides[0]["ids"][qy, qx, 3] == 1) & (np.linalg.norm(seen - eye, axis=-1) < far - 0.3)
        mask = got["motion"][..., 3]
        print(f"cornell box {W} x {H}, 6 degrees: {int(inside.sum())} pixels project into the previous frame, longest motion {moved.max():.2f} px; {int(other.sum())} of them were "
              f"hidden behind a nearer surface; tap masks: none {int((mask[inside] == 0).sum())}, all four {int((mask[inside] == 15).sum())}")
        assert other.sum() >= 10 and (mask[other] == 0).all() and (got["history"][other][:, 3] == 1.0).all()
        assert (mask[inside] == 15).mean() > 0.7
        a.buffer_free(d_image)
    finally:
        a.close(), b.close()


def test_an_orbit_of_twelve_poses_is_closer_to_the_converged_frame():
    from strelka_amd import capi

    W = H = 128
    POSES, STEP = 12, 1.0
    sc = scenes.cornell_box()
    arr = sc.arrays()
    c, truth = capi.Context(0), capi.Context(0)
    try:
        for x in (c, truth):
            x.set_scene(arr)
            x.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        prev, prev_aov = None, None
        for k in range(POSES):
            cam = orbit(sc.getCamera(), STEP * k)
            aov = S.aov_params(cam, W, H)
            guides = c.render_guides(aov)
            raw = sample_frame(c, cam, W, H, k, d_image)
            out = c.temporal(raw, guides, prev, S.temporal_params(W, H, prev_aov, scene=arr))
            prev = {"history": out["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}
            prev_aov = aov
        c.buffer_free(d_image)
        truth.render_subframes(S.frame_params(cam, W, H, subframe_index=0, spp_total=1024, max_depth=4), 1024)
        want = truth.read_accum()[..., :3].astype(np.float64)
        kind = guides["ids"][..., 3]
        surf = ((kind == 1) | (kind == 2)) & np.isfinite(raw[..., :3]).all(-1)
        rms = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - want)[surf] ** 2).mean()))
        dp = lambda img: S.denoise_params(W, H, scene=arr, image=img, guides=guides)
        e_raw, e_temporal = rms(raw), rms(out["image"])
        e_denoised, e_both = rms(c.denoise(raw, guides, dp(raw))), rms(c.denoise(out["image"], guides, dp(out["image"])))
        n = out["history"][..., 3][surf]
        print(f"cornell box {W} x {H}, pose {POSES} of an orbit in steps of {STEP} degrees, one sample per pose; rms error against 1024 spp over the surface pixels: raw {e_raw:.5f}, "
              f"temporal {e_temporal:.5f} (ratio {e_temporal / e_raw:.3f}), denoised {e_denoised:.5f}, temporal then denoised {e_both:.5f} (ratio {e_both / e_denoised:.3f}); "
              f"history length: mean {n.mean():.2f}, pixels at 1 {float((n == 1).mean()):.3f}")
        assert e_temporal < e_raw and e_both < e_denoised
    finally:
        c.close(), truth.close()
