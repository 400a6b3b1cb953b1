"""History rectification on the device (skh_rectify; DESIGN.md section 2, "History rectification").  The definition has no transcendental, so the device must
give the bits of its float32 restatement (tests/rectifyref.py: rectify32) on every word of all three outputs; the float64 reference with its written-out error
bar (rectify64) is the second, independent yardstick: r, the image, dmax and s0 on every pixel, the mask and n' on every pixel whose comparisons are decided
beyond the bar.  Chained behind skh_rewind_guides and two skh_temporal calls on a rendered scene it must give the bits of the chained restatements, and on a
block that moved it must bring the floor's history to the new shadow sooner than skh_temporal alone does.  Every test calls the new entry points, so each
fails without the feature.

Figures on an MI355X: docs/LOG.md has the lines the tests print."""

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import motionref as M
from tests import rectifyref as R
from tests import temporalref as T
from tests.denoiseref import modulation

pytestmark = pytest.mark.gpu

INPUTS = ("image", "ids", "albedo", "history", "fast")
OUTPUTS = ("out", "history_out", "info")
RADII = (1, 2, 3)
FLAGS = (0, R.REMODULATE, R.SHORTEN, R.REMODULATE | R.SHORTEN)
STEP = np.array([-0.30, 0.0, 0.15])  # the short block's translation


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Device:
    """device copies of one synthetic input (rectifyref.synthetic's dictionary) and three output planes"""

    def __init__(self, ctx, s):
        self.ctx, self.s = ctx, s
        self.h, self.w = s["ids"].shape[:2]
        self.d = {n: ctx.buffer_alloc(16 * self.w * self.h) for n in INPUTS + OUTPUTS}
        self.restore()

    def restore(self):
        for n in INPUTS:
            self.ctx.buffer_upload(self.d[n], self.s[n])

    def fill(self, name, value):
        self.ctx.buffer_upload(self.d[name], np.full((self.h, self.w, 4), value, np.float32))

    def download(self, name):
        out = np.zeros((self.h, self.w, 4), np.float32)
        self.ctx.buffer_download(self.d[name], out)
        return out

    def args(self, p, out="out", history_out="history_out", info=True, null=()):
        """the call's arguments; `out` / `history_out`: the planes written; `null`: the names of inputs or outputs handed over as NULL"""
        d = dict(self.d)
        d.update({n: None for n in null})
        return [p, d["image"], d["ids"], d["albedo"], d["history"], d["fast"], d[out], d[history_out], d["info"] if info else None]

    def run(self, p, out="out", history_out="history_out", info=True, null=()):
        self.ctx.rectify_device(*self.args(p, out, history_out, info, null))
        return {"image": self.download(out), "history": self.download(history_out), "info": self.download("info")}

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


def compare(d, p, label):
    """the device against both references: every word of the three outputs against float32, float64's bar under rectifyref.check's rules"""
    got = d.run(p)
    want, ref = R.rectify32(*R.planes(d.s), p), R.rectify64(*R.planes(d.s), p)
    differing = {n: int((bits(got[n]) != bits(want[n])).sum()) for n in got}
    worst, share = R.check(got, ref)
    print(f"{label}: words that differ from the float32 restatement {differing} of {4 * d.w * d.h} each; worst error / float64 bar {worst:.3f} over "
          f"{int(ref['rectified'].sum())} rectified pixels, ambiguous share {share:.5f}")
    for n in got:
        assert np.array_equal(bits(got[n]), bits(want[n])), (label, n)
    assert worst <= 1.0
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the bits, and the bar
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("radius", RADII)
def test_synthetic_bit_for_bit_and_inside_the_bar(dev, radius, flags):
    got, ref = compare(dev, R.params(67, 45, radius=radius, flags=flags), f"67 x 45, radius {radius}, flags {flags}")
    rect = ref["rectified"]
    assert (got["info"][rect][:, 0] != 0).mean() > 0.3 and (got["info"][rect][:, 0] == 0).sum() > 10  # (it clamped, and not everywhere)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63)])
def test_shapes_bit_for_bit(ctx, w, h):
    """one-row and one-column images, the image borders and the partial 64 x 4 workgroups"""
    d = Device(ctx, R.synthetic(w, h, seed=w + h))
    try:
        compare(d, R.params(w, h, radius=3), f"{w} x {h}, radius 3, both flags")
    finally:
        d.free()


def test_in_place_without_the_info_plane_and_infinite_k(dev):
    p = R.params(67, 45, radius=2)
    whole = dev.run(p)
    try:
        for out, history_out in (("image", "history_out"), ("out", "history"), ("image", "history")):
            dev.fill("info", 7.25)
            got = dev.run(p, out=out, history_out=history_out)
            for n in whole:
                assert np.array_equal(bits(got[n]), bits(whole[n])), (out, history_out, n)
            dev.restore()
        # no info plane: the other two outputs keep their bits, the info buffer is not written
        for n in OUTPUTS:
            dev.fill(n, 7.25)
        got = dev.run(p, info=False)
        assert np.array_equal(bits(got["image"]), bits(whole["image"])) and np.array_equal(bits(got["history"]), bits(whole["history"])) and (got["info"] == 7.25).all()
        # without REMODULATE the albedo plane may be NULL
        q = R.params(67, 45, radius=2, flags=R.SHORTEN)
        a, b = dev.run(q), dev.run(q, null=("albedo",))
        assert all(np.array_equal(bits(a[n]), bits(b[n])) for n in a)
        # k = +inf: both inputs come back, bit for bit, at every radius
        for radius in RADII:
            got = dev.run(R.params(67, 45, radius=radius, k=np.inf))
            assert np.array_equal(bits(got["image"]), bits(dev.s["image"])) and np.array_equal(bits(got["history"]), bits(dev.s["history"])), radius
            assert not got["info"][..., 0].any() and not got["info"][..., 2].any()
    finally:
        dev.restore()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_info_counts_accepted_calls(dev):
    from strelka_amd import capi

    c = capi.Context(0)
    d = Device(c, dev.s)
    good = R.params(67, 45, radius=2)

    def edited(**kw):
        q = np.array(good)
        for k, v in kw.items():
            if k == "reserved":
                q["reserved"][v] = 1
            else:
                q[k] = v
        return q

    records = {"zero width": edited(width=0), "zero height": edited(height=0), "more than 2^26 pixels": edited(width=(1 << 13) + 1, height=1 << 13),
               "radius 0": edited(radius=0), "radius 4": edited(radius=4), "k 0": edited(k=0.0), "k < 0": edited(k=-1.0), "k nan": edited(k=np.nan),
               "albedo_floor 0": edited(albedo_floor=0.0), "albedo_floor inf": edited(albedo_floor=np.inf), "albedo_floor nan": edited(albedo_floor=np.nan),
               "flag bit 2": edited(flags=7), "reserved[0]": edited(reserved=0), "reserved[7]": edited(reserved=7)}
    try:
        assert c.rectify_info() == {"calls": 0, "pixels": 0, "ms_last": 0.0}
        cases = {name: d.args(q) for name, q in records.items()}
        cases.update({"no " + n: d.args(good, null=(n,)) for n in ("image", "ids", "history", "fast", "out", "history_out")})
        cases["no albedo under REMODULATE"] = d.args(good, null=("albedo",))
        cases["the history written over the fast history"] = d.args(good, history_out="fast")
        cases["the image written over the fast history"] = d.args(good, out="fast")
        first = d.run(good)
        before = c.rectify_info()
        assert (before["calls"], before["pixels"]) == (1, 67 * 45) and before["ms_last"] > 0.0
        for n in OUTPUTS:
            d.fill(n, 7.25)
        for name, a in cases.items():
            assert not capi.rectify_check(a[0]) or name not in records, name
            with pytest.raises(capi.SkhError, match="skh_rectify"):
                c.rectify_device(*a)
            for n in OUTPUTS:
                assert (d.download(n) == 7.25).all(), (name, n)
            assert np.array_equal(bits(d.download("fast")), bits(d.s["fast"])), name
        after = c.rectify_info()
        assert (after["calls"], after["pixels"]) == (1, 67 * 45) and len(cases) == len(records) + 9
        again = d.run(good)
        assert all(np.array_equal(bits(again[n]), bits(first[n])) for n in first) and c.rectify_info()["calls"] == 2
        c.reset_stats()
        info = c.rectify_info()
        assert (info["calls"], info["pixels"]) == (0, 0)
    finally:
        d.free()
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. a rendered scene: the chain's bits, and a frame that does not notice
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sample_frame(c, cam, W, H, index, d_image):
    """one raw sample of the sequence as an image: the call HipRender makes for a restarted accumulation with temporal accumulation on"""
    c.render_subframe(S.frame_params(cam, W, H, subframe_index=index, spp_total=64, max_depth=4, enable_accumulation=0), d_image)
    out = np.zeros((H, W, 4), np.float32)
    c.buffer_download(d_image, out)
    return out


def translated(instances, index, t):
    inst = instances.copy()
    inst["transform"][index][[3, 7, 11]] += np.asarray(t, np.float32)
    return inst


def previous(history, guides):
    return {"history": history, "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}


def test_cornell_blocks_the_chain_bit_for_bit_and_the_frame_is_untouched():
    from strelka_amd import capi

    W, H = 96, 64
    SHORT = scenes.CORNELL_BLOCKS_SHORT
    sc = scenes.cornell_blocks()
    arr = sc.arrays()
    cam = sc.getCamera()
    rest, moved = arr["instances"], translated(arr["instances"], SHORT, STEP)
    a, b = capi.Context(0), capi.Context(0)
    try:
        for c in (a, b):
            c.set_scene(arr)
            c.resize(W, H)
        aov = S.aov_params(cam, W, H)
        tl = lambda prev_aov: S.temporal_params(W, H, prev_aov, scene=arr)
        tf = lambda prev_aov: S.temporal_params(W, H, prev_aov, max_history=S.RECTIFY_FAST_HISTORY, scene=arr)
        rp = S.rectify_params(W, H)
        # every device plane the chain touches exists before the first sub-frame: per frame the raw image and the four guide planes, then the rewound pair, two
        # long and two fast histories, the two temporal images, the rectified image and the info plane
        names = capi.DENOISE_GUIDES
        mask = sum(1 << S.AOV_PLANES.index(n) for n in names)
        alloc = lambda: a.buffer_alloc(16 * W * H)
        dev = [{n: alloc() for n in names + ("raw",)} for _ in range(4)]
        work = {n: alloc() for n in ("position", "normal", "long0", "long1", "fast0", "fast1", "image", "discard", "out", "info")}

        def download(d, dtype=np.float32):
            out = np.zeros((H, W, 4), dtype)
            a.buffer_download(d, out)
            return out

        # four frames of the sequence first: the block at rest, then three with it moved (render_aovs through the pixel centres, one raw sample)
        centre = np.array(aov)
        centre["x0"] = centre["y0"] = centre["width"] = centre["height"] = 0
        centre["sample_index"] = S.AOV_PIXEL_CENTRE
        frames = []
        for k in range(4):
            if k == 1:
                for c in (a, b):
                    c.update_accel(moved)
            a.render_aovs_device(centre, mask, [dev[k].get(n) for n in S.AOV_PLANES])
            a.render_subframe(S.frame_params(cam, W, H, subframe_index=k, spp_total=64, max_depth=4, enable_accumulation=0), dev[k]["raw"])
            frames.append(({n: download(dev[k][n], np.uint32 if n == "ids" else np.float32) for n in names}, download(dev[k]["raw"])))
        # an accumulation in progress, beside a context that never hears of the feature
        for c in (a, b):
            for i in range(3):
                c.render_subframe(S.frame_params(cam, W, H, subframe_index=i, spp_total=64, max_depth=4))
        accum, stats, adaptive = a.read_accum(), a.stats(), a.adaptive_info()
        d, (guides, raw) = dev[0], frames[0]
        for p, hist in ((tl(None), "long0"), (tf(None), "fast0")):
            a.temporal_device(p, d["raw"], d["ids"], d["normal"], d["position"], d["albedo"], None, None, None, None, work["discard"], work[hist], None)
        long_, fast = download(work["long0"]), download(work["fast0"])
        assert np.array_equal(bits(long_), bits(T.reproject32(raw, guides["ids"], guides["normal"], guides["position"], guides["albedo"], None, tl(None))["history"]))
        stored = 0
        poses = [rest, moved, moved, moved]
        clamped = []
        for k in (1, 2, 3):
            prev_guides, pd = guides, d
            d, (guides, raw) = dev[k], frames[k]
            table = S.instance_motion(poses[k - 1], poses[k])
            a.set_instance_motion(table)
            a.rewind_guides_device(W, H, d["ids"], d["position"], d["normal"], work["position"], work["normal"])
            nxt = 1 - stored
            for p, hist, image in ((tl(aov), "long", "image"), (tf(aov), "fast", "discard")):
                a.temporal_device(p, d["raw"], d["ids"], work["normal"], work["position"], d["albedo"], work[f"{hist}{stored}"], pd["ids"], pd["normal"], pd["position"],
                                  work[image], work[f"{hist}{nxt}"], None)
            a.rectify_device(rp, work["image"], d["ids"], d["albedo"], work[f"long{nxt}"], work[f"fast{nxt}"], work["out"], work[f"long{nxt}"], work["info"])
            stored = nxt
            got = {"image": download(work["out"]), "history": download(work[f"long{stored}"]), "info": download(work["info"])}
            got_fast = download(work[f"fast{stored}"])
            want_rw = M.rewind32(guides["ids"], guides["position"], guides["normal"], table)
            wt = T.reproject32(raw, guides["ids"], want_rw["normal"], want_rw["position"], guides["albedo"], previous(long_, prev_guides), tl(aov))
            wf = T.reproject32(raw, guides["ids"], want_rw["normal"], want_rw["position"], guides["albedo"], previous(fast, prev_guides), tf(aov))
            want = R.rectify32(wt["image"], guides["ids"], guides["albedo"], wt["history"], wf["history"], rp)
            assert np.array_equal(bits(got_fast), bits(wf["history"])), k
            for n in ("image", "history", "info"):
                assert np.array_equal(bits(got[n]), bits(want[n])), (k, n)
            long_, fast = want["history"], wf["history"]
            clamped.append(int((got["info"][..., 0] != 0).sum()))
        print(f"cornell blocks {W} x {H}, the short block translated by {tuple(STEP.tolist())}: pixels with a clamped channel in the three frames after the step {clamped}")
        assert min(clamped) > 0
        # the frame did not move
        after = a.stats()
        assert np.array_equal(bits(a.read_accum()), bits(accum)) and a.adaptive_info() == adaptive
        assert all(after[k] == stats[k] for k in after if k.startswith("rays_") or k.startswith("launches_")) and after["speculated_discarded"] == stats["speculated_discarded"]
        for c in (a, b):
            c.render_subframe(S.frame_params(cam, W, H, subframe_index=3, spp_total=64, max_depth=4))
        assert np.array_equal(bits(a.read_accum()), bits(b.read_accum()))
        info = a.rectify_info()
        assert (info["calls"], info["pixels"]) == (3, 3 * W * H) and info["ms_last"] > 0.0 and b.rectify_info()["calls"] == 0
        for x in dev + [work]:
            for v in x.values():
                a.buffer_free(v)
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. quality: the floor under a block that moved
# ---------------------------------------------------------------------------------------------------------------------------------------------
def quality_sequence(configs, W=128, H=128, rest_frames=16, moved_frames=12, report=(1, 2, 4, 8, 12), reference_spp=1024, own_context=True):
    """cornell_blocks with a still camera at one sample per frame: `rest_frames` with the short block at rest, then `moved_frames` with it translated by STEP.
    `configs`: name -> (radius, k, shorten, fast_length).  -> {"masks": {"changed": n, "unchanged": n}, "rms": {name or "temporal" or "temporal_fast<n>" (the fast history alone) or "raw": {frames after the
    step: (changed, unchanged)}}, "clamped": {name: {frames after the step: (changed, unchanged)}}}: the share of pixels with a clamped channel, and the rms error of the output image's rgb against `reference_spp` samples of the new pose, over the static surface pixels outside the
    block in both poses, split by whether the two references' demodulated luminance differs by more than a quarter of its mean."""
    from strelka_amd import capi

    SHORT = scenes.CORNELL_BLOCKS_SHORT
    sc = scenes.cornell_blocks()
    arr = sc.arrays()
    cam = sc.getCamera()
    rest, moved = arr["instances"], translated(arr["instances"], SHORT, STEP)
    # (the image passes run on a context of their own, `post`, which traces nothing: the figures then do not depend on what the rendering context has in flight.
    # own_context=False is the experiment of docs/LOG.md, "History rectification": the numpy forms allocate a buffer per plane and call, beside a pass traced ahead)
    c, truth = capi.Context(0), [capi.Context(0), capi.Context(0)]
    post = capi.Context(0) if own_context else c
    try:
        for x in [c] + truth:
            x.set_scene(arr)
            x.resize(W, H)
        truth[1].update_accel(moved)
        refs = []
        for x in truth:
            x.render_subframes(S.frame_params(cam, W, H, subframe_index=0, spp_total=reference_spp, max_depth=4), reference_spp)
            refs.append(x.read_accum()[..., :3].astype(np.float64))
        d_image = c.buffer_alloc(16 * W * H)
        aov = S.aov_params(cam, W, H)
        fast_lengths = sorted({cfg[3] for cfg in configs.values()})
        hist = {name: None for name in list(configs) + ["temporal"] + [("fast", n) for n in fast_lengths]}
        rms = {name: {} for name in list(configs) + ["temporal", "raw"] + [f"temporal_fast{int(n)}" for n in fast_lengths]}
        clamped = {name: {} for name in configs}
        guides, masks = None, None
        for k in range(rest_frames + moved_frames):
            prev_guides = guides
            if k == rest_frames:
                c.update_accel(moved)
            guides = c.render_guides(aov)
            kind = guides["ids"][..., 3]
            static = ((kind == 1) | (kind == 2)) & (guides["ids"][..., 0] != SHORT)
            if k == 0:
                static_at_rest = static
            raw = sample_frame(c, cam, W, H, k, d_image)
            g = guides
            if k == rest_frames:  # the block's own pixels follow it (skh_rewind_guides); the floor's do not move
                post.set_instance_motion(S.instance_motion(rest, moved))
                rw = post.rewind_guides(guides)
                g = dict(guides, position=rw["position"], normal=rw["normal"])
                m = modulation(guides["albedo"], S.DENOISE_ALBEDO_FLOOR).astype(np.float64)
                lum = [S.luminance(r / m) for r in refs]
                both = static & static_at_rest & np.isfinite(raw[..., :3]).all(-1)
                changed = both & (np.abs(lum[1] - lum[0]) > 0.25 * lum[1][both].mean())
                masks = {"changed": changed, "unchanged": both & ~changed}
            tp = lambda n: S.temporal_params(W, H, aov if k else None, max_history=n, scene=arr)
            prev = lambda name: None if k == 0 else previous(hist[name], prev_guides)
            out, info = {"raw": raw}, {}
            for n in fast_lengths:
                t = post.temporal(raw, g, prev(("fast", n)), tp(n))
                hist[("fast", n)], out[f"temporal_fast{int(n)}"] = t["history"], t["image"]
            t = post.temporal(raw, g, prev("temporal"), tp(S.TEMPORAL_MAX_HISTORY))
            hist["temporal"], out["temporal"] = t["history"], t["image"]
            for name, (radius, kk, shorten, n) in configs.items():
                t = post.temporal(raw, g, prev(name), tp(S.TEMPORAL_MAX_HISTORY))
                r = post.rectify(t["image"], guides, t["history"], hist[("fast", n)], S.rectify_params(W, H, radius=radius, k=kk, shorten=shorten))
                hist[name], out[name], info[name] = r["history"], r["image"], r["info"]
            after = k - rest_frames + 1
            if after in report:
                for name, img in out.items():
                    err = (img[..., :3].astype(np.float64) - refs[1]) ** 2
                    rms[name][after] = tuple(float(np.sqrt(err[masks[region]].mean())) for region in ("changed", "unchanged"))
                for name, plane in info.items():
                    clamped[name][after] = tuple(float((plane[..., 0][masks[region]] != 0).mean()) for region in ("changed", "unchanged"))
        c.buffer_free(d_image)
        return {"masks": {n: int(v.sum()) for n, v in masks.items()}, "rms": rms, "clamped": clamped}
    finally:
        c.close()
        if post is not c:
            post.close()
        for x in truth:
            x.close()


def test_the_floor_under_a_moved_block_follows_the_new_shadow_sooner():
    """Orderings only, 8 frames after the step: the changed region's rms error with rectification below that without, the unchanged region's below the raw frame's.
    Measured on an MI355X (docs/LOG.md): rectified 0.0203 / 0.0116, skh_temporal alone 0.0500 / 0.0111, the raw frame 0.0456 / 0.0978."""
    q = quality_sequence({"rectified": (S.RECTIFY_RADIUS, S.RECTIFY_K, S.RECTIFY_SHORTEN_DEFAULT, S.RECTIFY_FAST_HISTORY)}, report=(8,))
    (rc, ru), (tc, tu), (wc, wu) = q["rms"]["rectified"][8], q["rms"]["temporal"][8], q["rms"]["raw"][8]
    print(f"cornell blocks 128 x 128, the short block translated by {tuple(STEP.tolist())} after 16 frames at rest, 8 frames after the step, rms error against 1024 spp "
          f"(changed {q['masks']['changed']} pixels / unchanged {q['masks']['unchanged']}): raw frame {wc:.4f} / {wu:.4f}, temporal {tc:.4f} / {tu:.4f}, "
          f"rectified (radius {S.RECTIFY_RADIUS}, k {S.RECTIFY_K}, fast history {S.RECTIFY_FAST_HISTORY}) {rc:.4f} / {ru:.4f}")
    assert q["masks"]["changed"] > 100 and q["masks"]["unchanged"] > 5000
    assert rc < tc and ru < wu
