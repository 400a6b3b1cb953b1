"""The environment (dome) light on the GPU ("Environment light").  The CPU checker knows no environment, so nothing here is
"HIP == oracle": the device functions are held against the float64 restatement in tests/envref.py through the unit probes (which call the
`__device__` functions k_shade calls), against exact identities, and the integrator against closed forms with bounds DERIVED from the input map.

eps(n) = (n + 8) 2^-24: the worst relative error of an fp32 sum of n non-negative terms in any order plus the few roundings inside one weight; a CDF
is <= 1, so it is an absolute bound too.  (The tables are summed in double: the bound is met with room, it is not tuned to them.)"""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes, tiles
from tests import envref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # half an ulp, relative


def eps(n):
    return (n + 8) * U


@pytest.fixture(scope="module")
def gpu():
    from strelka_amd import build, capi

    build.build()
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def ctx():
    from strelka_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def sample(gpu, u):
    o = gpu.unit_probe("env_sample", np.ascontiguousarray(u, np.float32))
    return {"dir": f32(o[:, 0:3]), "pdf": f32(o[:, 3:4])[:, 0], "Le": f32(o[:, 4:7]), "ix": o[:, 7].astype(np.int64), "iy": o[:, 8].astype(np.int64)}


def evaluate(gpu, d):
    o = gpu.unit_probe("env_eval", np.ascontiguousarray(d, np.float32))
    return {"Le": f32(o[:, 0:3]), "pdf": f32(o[:, 3:4])[:, 0], "ix": o[:, 4].astype(np.int64), "iy": o[:, 5].astype(np.int64)}


QUARTER = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)  # a quarter turn about Y, entries 0 and +-1: exact in fp32


def check_eval_against_float64(rgb, scale, d, got, w2e=None):
    """Le bit-equal to scale * texel; the texel = the float64 one, or its neighbour where the direction lies within rounding of an edge; pdf at the bar
    written out below.  `w2e` must be exact in fp32 (identity / quarter turns): the bar has no term for a rotation's roundings."""
    H, W = rgb.shape[:2]
    x, y = envref.texel_coords(d, W, H, w2e)
    # coordinate error: atan2 <= 3.5 ulp (tests/test_libm.py), acos <= 1.3 ulp, the (+ 2 pi) and the two multiplications half an ulp each
    tx, ty = W * (3.5 + 0.5 + 1.0) * 2 * U, H * (1.3 + 1.0) * 2 * U
    okx = (got["ix"] == np.minimum(np.floor(x - tx) % W, W - 1)) | (got["ix"] == np.minimum(np.floor(x + tx) % W, W - 1)) | (got["ix"] == np.minimum(np.floor(x), W - 1))
    oky = (got["iy"] == np.clip(np.floor(y - ty), 0, H - 1)) | (got["iy"] == np.clip(np.floor(y + ty), 0, H - 1))
    assert okx.all() and oky.all(), (int((~okx).sum()), int((~oky).sum()))
    ex, ey = envref.texel_of(d, W, H, w2e)
    edge = float(((got["ix"] != ex) | (got["iy"] != ey)).mean())
    want_le = (np.asarray(scale, np.float32)[None, :] * rgb[got["iy"], got["ix"]]).astype(np.float32)
    assert np.array_equal(got["Le"].view(np.uint32), want_le.view(np.uint32))
    want = envref.pdf(rgb, d, got["ix"], got["iy"], w2e)
    # the bar, as a sum: w / sum w (sum of W terms, then of H row sums; its one stored rounding is in the + 8) ...
    bar = eps(W) + eps(H)
    bar += 6 * U  # ... half an ulp for each fp32 operation of (p * pdfScale) / sqrt(x * x + z * z): two products, a sum, a root, a product, a quotient
    bar += 1 * U  # ... and the rounding of the constant W H / (2 pi^2)
    rel = np.abs(got["pdf"].astype(np.float64) - want) / np.maximum(want, 1e-300)
    print(f"env_eval {W}x{H}: pdf relative error max {rel[want > 0].max():.3e} (bar {bar:.3e}), {edge:.2e} of the directions in an edge neighbour")
    assert (rel[want > 0] <= bar).all() and (got["pdf"][want == 0] == 0).all()
    return edge


@pytest.mark.parametrize("W,H", [(64, 32), (512, 256), (2048, 1024)])
def test_sampler_and_eval_against_float64(gpu, W, H):
    rgb = envref.sky_map(W, H, seed=W)
    scale = (1.5, 1.0, 0.25)
    gpu.set_environment(rgb, scale)
    info = gpu.environment_info()
    marg, cond, total = envref.cdfs(rgb)
    assert (info["width"], info["height"]) == (W, H) and abs(info["sum_w"] / total - 1) <= eps(W) + eps(H) and info["bytes"] == W * H * 20 + H * 4
    u = np.random.RandomState(11).rand(100000, 2).astype(np.float32)
    u[:8] = [(0, 0), (0.99999994, 0.99999994), (0, 0.99999994), (0.99999994, 0), (0.5, 0.5), (1e-7, 1e-7), (0.25, 0.75), (0.75, 0.25)]
    s = sample(gpu, u)
    assert (s["ix"] < W).all() and (s["iy"] < H).all()
    u1, u2 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    lo, hi = marg[s["iy"]], marg[s["iy"] + 1]
    assert ((lo - eps(H) <= u1) & (u1 <= hi + eps(H))).all()
    clo, chi = cond[s["iy"], s["ix"]], cond[s["iy"], s["ix"] + 1]
    assert ((clo - eps(W) <= u2) & (u2 <= chi + eps(W))).all()
    # the sun takes most of the samples, and a texel of weight 0 none: every selected texel has w > 0
    assert (envref.weights(rgb)[s["iy"], s["ix"]] > 0).all()
    # env_eval: random directions, the poles, the seam, axis directions
    d = np.concatenate([envref.random_directions(100000, 5), np.float32([(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 0, -1e-9), (1, 1e-9, 1e-9)])])
    check_eval_against_float64(rgb, scale, d, evaluate(gpu, d))
    # normalisation over the texel centres: sum pdf 2 pi^2 sin(theta) / (W H) = sum w / sum w = 1, at the same bar
    if W <= 512:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        t, f = np.pi * (yy.ravel() + 0.5) / H, 2 * np.pi * (xx.ravel() + 0.5) / W
        dirs = np.stack([np.sin(t) * np.cos(f), np.cos(t), np.sin(t) * np.sin(f)], 1).astype(np.float32)
        e = evaluate(gpu, dirs)
        assert np.array_equal(e["ix"], xx.ravel()) and np.array_equal(e["iy"], yy.ravel())
        l = dirs.astype(np.float64)
        tot = float((e["pdf"].astype(np.float64) * 2 * np.pi ** 2 * np.hypot(l[:, 0], l[:, 2]) / (W * H)).sum())
        print(f"normalisation {W}x{H}: {tot - 1:+.3e}")
        assert abs(tot - 1) <= eps(W) + eps(H) + 7 * U


@pytest.mark.parametrize("W,H", [(64, 32), (2048, 1024)])
def test_sample_and_eval_agree(gpu, W, H):
    rgb = envref.sky_map(W, H, seed=3)
    R = QUARTER
    for w2e in (None, R):
        gpu.set_environment(rgb, (1, 2, 3), w2e)
        u = np.random.RandomState(2).rand(200000, 2).astype(np.float32)
        s = sample(gpu, u)
        e = evaluate(gpu, s["dir"])
        assert np.array_equal(e["Le"].view(np.uint32), s["Le"].view(np.uint32)) and np.array_equal(e["pdf"].view(np.uint32), s["pdf"].view(np.uint32))
        assert abs(np.linalg.norm(s["dir"].astype(np.float64), axis=1) - 1).max() <= 8 * U
        dx, dy = (e["ix"] - s["ix"]) % W, e["iy"] - s["iy"]
        dx = np.where(dx > W // 2, dx - W, dx)
        off = (dx != 0) | (dy != 0)
        assert (np.abs(dx) <= 1).all() and (np.abs(dy) <= 1).all()  # a mismatch is an ADJACENT texel
        print(f"sample -> eval {W}x{H}: {off.mean():.2e} of the samples land in a neighbour")
        assert off.mean() <= 1e-3
        # the direction the sampler returns lies in the texel it selected (float64 coordinates, the same edge tolerance as above)
        x, y = envref.texel_coords(s["dir"], W, H, w2e)
        xw = (x - (s["ix"] + 0.5) + W / 2) % W - W / 2  # (across the seam)
        assert (np.abs(xw) <= 0.5 + W * 16 * U).all() and (np.abs(y - (s["iy"] + 0.5)) <= 0.5 + H * 16 * U).all()


def test_exact_rotation(gpu):
    W, H = 512, 256
    rgb = envref.sky_map(W, H, seed=9)
    d = envref.random_directions(10000, 6)
    gpu.set_environment(rgb, (1, 1, 1), QUARTER)
    a = evaluate(gpu, d)
    gpu.set_environment_transform((1, 1, 1), None)
    b = evaluate(gpu, (d.astype(np.float64) @ QUARTER.astype(np.float64).T).astype(np.float32))  # R d: a permutation with a sign, exact
    for k in ("Le", "pdf"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    assert np.array_equal(a["ix"], b["ix"]) and np.array_equal(a["iy"], b["iy"])
    c = evaluate(gpu, d)
    assert not np.array_equal(a["ix"], c["ix"])  # and the rotation does something
    check_eval_against_float64(rgb, (1, 1, 1), d, a, QUARTER)


def empty_scene(cam_from=(0, 0, 0), cam_at=(0, 0, -1)):
    sc = S.Scene()
    cam = S.Camera(fov=60.0)
    cam.lookAt(cam_from, cam_at)
    sc.addCamera(cam)
    return sc


def render(ctx, sc, w, h, n, depth=4, **kw):
    ctx.resize(w, h)
    for i in range(n):
        ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=n, max_depth=depth, **kw))
    return ctx.read_accum()[..., :3]


def test_empty_scene_shows_the_map(ctx):
    sc = empty_scene()
    c = np.float32([0.7, 0.2, 1.9])
    sc.setEnvironment(np.broadcast_to(c, (8, 16, 3)).copy())
    ctx.set_scene(sc.arrays())
    n = 5
    img = render(ctx, sc, 32, 24, n)
    e = S.default_exposure()
    want = f32(ctx.unit_probe("accumulate", np.broadcast_to(c, (n, 3)).copy(), param=0, consts=np.ascontiguousarray(e, np.float32)))[n - 1]
    assert np.array_equal(img.view(np.uint32), np.broadcast_to(want, img.shape).copy().view(np.uint32))
    assert ctx.stats()["rays_shadow"] == 0  # nothing was hit: no light pick
    # two colours, camera level: rows above / below the horizon carry them (row 0 of the accumulator = launch y 0; which end is up is the camera's business)
    up, down = np.float32([1, 0, 0]), np.float32([0, 0, 1])
    m = np.zeros((8, 16, 3), np.float32)
    m[:4], m[4:] = up, down
    ctx.set_environment(m)
    img = render(ctx, sc, 32, 25, 1)
    first, last = img[0, 0], img[-1, 0]
    assert not np.array_equal(first, last) and {tuple(np.sign(first)), tuple(np.sign(last))} == {(1, 0, 0), (0, 0, 1)}
    for row in range(25):
        if row != 12:  # the horizon row may carry either
            assert (img[row] == (first if row < 12 else last)).all(), row
    assert all(((img[12, x] == first).all() or (img[12, x] == last).all()) for x in range(32))


def box_room(open_wall=False):
    """camera and a diffuse floor inside a closed 4 x 4 x 4 box (six quads facing inwards or not: an any-hit ray does not care)"""
    sc = S.Scene()
    grey = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    a = 2.0
    quads = [[(-a, -a, a), (a, -a, a), (a, -a, -a), (-a, -a, -a)], [(-a, a, -a), (a, a, -a), (a, a, a), (-a, a, a)],
             [(-a, -a, -a), (a, -a, -a), (a, a, -a), (-a, a, -a)], [(a, -a, a), (-a, -a, a), (-a, a, a), (a, a, a)],
             [(-a, -a, a), (-a, -a, -a), (-a, a, -a), (-a, a, a)], [(a, -a, -a), (a, -a, a), (a, a, a), (a, a, -a)]]
    if open_wall:
        quads = quads[:1] + quads[2:]  # no ceiling
    for q in quads:
        vb, ib = S.deindex(np.array(q, np.float32), np.array([(0, 1, 2), (0, 2, 3)]))
        sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), grey, np.eye(4))
    cam = S.Camera(fov=60.0)
    cam.lookAt((0.0, 0.5, 1.5), (0.0, -2.0, 0.0))
    sc.addCamera(cam)
    return sc


def test_closed_room_stays_black_and_an_open_one_does_not(ctx):
    sky = envref.sky_map(64, 32, seed=4)
    sc = box_room()
    sc.setEnvironment(sky)
    ctx.set_scene(sc.arrays())
    ctx.reset_stats()
    img = render(ctx, sc, 32, 32, 16, depth=4)
    st = ctx.stats()
    assert (img == 0).all() and st["rays_shadow"] > 0  # the environment's shadow rays were traced, and every one was occluded
    sc2 = box_room(open_wall=True)
    sc2.setEnvironment(sky)
    ctx.set_scene(sc2.arrays())
    img2 = render(ctx, sc2, 32, 32, 16, depth=4)
    assert np.isfinite(img2).all() and (img2 > 0).mean() > 0.9


def floor_scene(with_light, light_below=False):
    """the floor, material and camera of tests/test_oracle_render.py::floor_under_rect_light, with its light, with none, or with one UNDER the floor facing down"""
    from tests.test_oracle_render import floor_under_rect_light

    full, want = floor_under_rect_light()
    if with_light:
        return full, want
    rho = 0.5
    sc = S.Scene()
    grey = sc.addMaterial(S.MAT_DIFFUSE, (rho, rho, rho))
    vb, ib = S.deindex(np.array([(-20, 0, 20), (20, 0, 20), (20, 0, -20), (-20, 0, -20)], np.float32), np.array([(0, 1, 2), (0, 2, 3)]))
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), grey, np.eye(4))
    if light_below:
        xf = S.translate((0.0, -1.5, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # emits towards -Y, away from the floor above it
        sc.createLight({"type": 0, "xform": xf, "useXform": True, "width": 1.0, "height": 0.6, "color": (10.0, 10.0, 10.0), "intensity": 1.0})
    cam = S.Camera(fov=1.5)
    cam.lookAt((3.0, 1.0, 0.4), (0.0, 0.0, 0.0))
    sc.addCamera(cam)
    return sc, 0.0


def one_launch(ctx, sc, spp, depth, **kw):
    ctx.resize(8, 8)
    ctx.render_subframe(S.frame_params(sc.getCamera(), 8, 8, subframe_index=0, samples_this_launch=spp, spp_total=spp, max_depth=depth, **kw))
    return ctx.read_accum()[..., :3].astype(np.float64)


MSE_LOG = {}


@pytest.mark.parametrize("light_below", [False, True])
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("sun", [False, True])
def test_floor_under_a_sky_has_its_closed_form(ctx, sun, depth, light_below):
    """A floor point sees the whole upper hemisphere and nothing it reflects comes back: every pixel's expectation is mu = rho E_cos[Le] (exact for the
    piecewise-constant map).  One launch of N samples, the mean over the P pixels, per channel: |mean - mu| <= 6 sqrt(V / (P N)), V = V0 = rho^2 E_cos[Le^2] - mu^2
    for env_nee 0 (cosine sampling) and V0 + mu^2 / 2 for the default (Veach's bound for the balance heuristic with one sample per technique).  A light
    under the floor lights nothing -- mu and the bounds stay -- but takes half the picks: a wrong 1 / (numLights + 1) would bias the NEE share."""
    rho, N, P = 0.5, 1024, 64
    rgb = envref.sky_map(256, 128, seed=21) if sun else np.broadcast_to(np.float32([0.6, 0.3, 0.9]), (16, 32, 3)).copy()
    scale = np.float32([1.0, 0.5, 2.0])
    m1, m2 = envref.cosine_moments(rgb, scale)
    mu, V0 = rho * m1, rho ** 2 * m2 - (rho * m1) ** 2
    sc, _ = floor_scene(False, light_below)
    sc.setEnvironment(rgb, scale)
    ctx.set_scene(sc.arrays())
    mse = {}
    for nee in (0, 1):
        ctx.set_option("env_nee", nee)
        ctx.reset_stats()
        img = one_launch(ctx, sc, N, depth)
        mean = img.mean(axis=(0, 1))
        V = V0 + (mu ** 2 / 2 if nee else 0.0)
        bound = 6 * np.sqrt(np.maximum(V, 0) / (P * N)) + eps(N) * mu  # (+ eps(N): the fp32 sum of the N samples -- all that separates a constant map's env_nee 0 mean from mu, V0 being 0)
        mse[nee] = float(((img - mu) ** 2).mean())
        print(f"sun {sun} depth {depth} below {light_below} env_nee {nee}: mean {mean}, mu {mu}, |diff| / bound {np.abs(mean - mu) / bound}, per-pixel MSE {mse[nee]:.4e}, shadow rays {ctx.stats()['rays_shadow']}")
        assert (np.abs(mean - mu) <= bound).all(), (nee, mean, mu, bound)
        assert (ctx.stats()["rays_shadow"] > 0) == bool(nee)
    MSE_LOG[(sun, depth, light_below)] = mse
    if sun:
        assert mse[1] < mse[0], mse  # importance sampling the sun beats waiting for the BSDF to find it


@pytest.mark.parametrize("method", [0, 1])
def test_floor_under_a_rect_light_and_a_constant_sky(ctx, method):
    """floor_under_rect_light() as it is plus a constant map c: mu = the light's closed form + rho c (1 - 1 / pi Integral_rect H^2 / r^4 dA) -- the sky
    minus the part the light's proxy hides -- at that test's bar, 1.5 % at 65 536 samples.  The leg that runs the light-hit branch with numLights + 1."""
    sc, want = floor_scene(True)
    rho, Hh, a, b, c = 0.5, 1.5, 1.0, 0.6, 2.0
    n = 1200
    xs, zs = (np.arange(n) + 0.5) / n * a - a / 2, (np.arange(n) + 0.5) / n * b - b / 2
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    hidden = float((Hh ** 2 / (X * X + Z * Z + Hh * Hh) ** 2).sum() * (a / n) * (b / n)) / math.pi
    mu = want + rho * c * (1 - hidden)
    sc.setEnvironment(np.full((16, 32, 3), c, np.float32))
    ctx.set_scene(sc.arrays())
    for nee in (1, 0):
        ctx.set_option("env_nee", nee)
        got = float(one_launch(ctx, sc, 1024, 2, rect_light_sampling_method=method).mean())
        print(f"rect light + sky, method {method}, env_nee {nee}: {got} against {mu} ({got / mu - 1:+.3%}; light alone {want}, hidden share {hidden:.4f})")
        assert abs(got - mu) <= 0.015 * mu, (method, nee, got, mu)


def test_nothing_changes_without_an_environment(gpu):
    from tests.test_gpu_parity import _render_both, _image_equal

    sc = scenes.cornell_box()
    gpu.set_environment(envref.sky_map(64, 32, seed=1))
    gpu.set_scene({**sc.arrays(), "environment": {"rgb": envref.sky_map(64, 32, seed=1)}})
    lit = render(gpu, sc, 48, 48, 2)
    gpu.set_environment(None)
    assert gpu.environment_info()["width"] == 0
    o, want, got = _render_both(gpu, sc, 48, 48, 4, 4)  # (set_scene without the entry: no environment either)
    _image_equal(got, want)
    assert not np.array_equal(lit, render(gpu, sc, 48, 48, 2))


def test_options_leave_an_environment_lit_image_bit_identical(ctx):
    import torch

    sc = scenes.cornell_box()
    sc.setEnvironment(envref.sky_map(256, 128, seed=8), (0.5, 0.5, 0.5), QUARTER)
    arr = sc.arrays()
    ctx.set_scene(arr)
    w, h, spp = 64, 48, 12

    def frame(batch=None):
        ctx.resize(w, h)
        if batch is None:
            return render(ctx, sc, w, h, spp).copy()
        ctx.render_subframes(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=spp, max_depth=4), spp)
        return ctx.read_accum()[..., :3].copy()

    ctx.set_option("speculate", 0)
    base = frame()
    assert base.max() > 0
    ctx.set_option("speculate", 8)
    assert np.array_equal(frame(), base)
    for b in (1, 5):
        ctx.set_option("subframe_batch", b)
        assert np.array_equal(frame(batch=True), base), b
    ctx.set_option("subframe_batch", 0)
    # tile sharding: two "ranks" on one GPU, every one given the same scene and environment
    full = np.zeros((h, w, 3), np.float32)
    T = 16
    for rank in range(2):
        txy = tiles.assign_tiles(w, h, T, 2, rank)
        ctx.set_tiles(T, txy)
        part = frame()
        for (x0, y0) in np.asarray(txy).reshape(-1, 2):
            full[y0:y0 + T, x0:x0 + T] = part[y0:y0 + T, x0:x0 + T]
    ctx.set_tiles(32, None)
    assert np.array_equal(full, base)
    # a transform between two sub-frames of a speculated frame shows in the very next one
    ctx.set_option("speculate", 8)
    ctx.resize(w, h)
    ctx.reset_stats()
    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    P = lambda i: S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=spp, max_depth=4)
    for i in range(5):
        ctx.render_subframe(P(i), img.data_ptr())
    ctx.set_environment_transform((4.0, 0.0, 0.0), None)
    ctx.render_subframe(P(5), img.data_ptr())
    with_spec = ctx.read_accum()[..., :3].copy()
    assert ctx.stats()["speculated_discarded"] > 0
    ctx.set_option("speculate", 0)
    ctx.set_environment_transform((0.5, 0.5, 0.5), QUARTER)
    ctx.resize(w, h)
    for i in range(5):
        ctx.render_subframe(P(i))
    ctx.set_environment_transform((4.0, 0.0, 0.0), None)
    ctx.render_subframe(P(5))
    assert np.array_equal(ctx.read_accum()[..., :3], with_spec)
    ctx.set_option("speculate", 8)


def test_bad_input_is_refused_and_the_context_stays_usable(ctx):
    from strelka_amd import capi

    sc = scenes.cornell_box()
    ctx.set_scene(sc.arrays())
    with pytest.raises(capi.SkhError, match="no environment"):
        ctx.set_environment_transform((1, 1, 1), None)
    with pytest.raises(capi.SkhError, match="no environment"):
        ctx.unit_probe("env_eval", np.float32([[0, 1, 0]]))
    good = envref.sky_map(32, 16, seed=2)
    for bad, what in ((np.where(np.arange(32 * 16 * 3).reshape(16, 32, 3) == 100, np.nan, good), "non-finite"),
                      (np.where(np.arange(32 * 16 * 3).reshape(16, 32, 3) == 7, -1.0, good), "negative"),
                      (np.where(np.arange(32 * 16 * 3).reshape(16, 32, 3) == 1500, np.inf, good), "non-finite"),
                      (good[:, :1], "wide"), (np.zeros((4097, 2, 3), np.float32), "high"), (good[:1], "high")):
        with pytest.raises(capi.SkhError, match=what) as ei:
            ctx.set_environment(bad.astype(np.float32))
        assert "(3)" in str(ei.value)  # SKH_INVALID_ARGUMENT
    assert ctx.environment_info()["width"] == 0
    ctx.set_environment(good)
    with pytest.raises(capi.SkhError):
        ctx.set_environment(np.full((16, 32, 3), np.nan, np.float32))
    with pytest.raises(capi.SkhError):
        ctx.set_environment_transform((np.nan, 1, 1), None)
    assert ctx.environment_info()["width"] == 32  # a refused map leaves the one in use
    a = render(ctx, sc, 32, 32, 2)
    ctx.set_environment(np.zeros((16, 32, 3), np.float32))  # all black: legal; never wins a shadow ray
    ctx.reset_stats()
    b = render(ctx, sc, 32, 32, 2)
    ctx.set_environment(None)
    c = render(ctx, sc, 32, 32, 2)
    assert np.isfinite(a).all() and not np.array_equal(a, b) and np.isfinite(b).all() and np.isfinite(c).all()
