"""The multi-bounce integrator against closed-form furnace radiances ("The integrator against the furnace").  A closed 2 x 2 x 2 room whose
walls all have one Lambertian albedo rho and emit one radiance Le inwards has the radiance Le sum rho^k in every direction at every point, and lossless objects put
into it change nothing.  tests/furnaceref.py writes down in float64 what the bounce loop makes of that -- the depth limit, the roulette and its 1 / (p + 1e-5)
rescale, the last vertex that is never shaded --; nothing here compares the GPU with the checker, which knows neither emission nor the environment nor blending.

U = 2^-24 is half an ulp, relative; eps(n) = (n + 8) U the in-launch mean of n samples (n - 1 sums, a quotient, the accumulate step), as in the neighbouring files.
Every bar below is a derived bound or a stated condition asserted on the inputs; none is fitted to what the device returns."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from tests import furnaceref as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LE = np.float32([1.0, 0.6, 0.3])
RHO_COLOUR = np.float32([0.3, 0.5, 0.8])
EYE, AT, FOV = (0.55, 0.35, 0.7), (-0.6, -0.25, -1.0), 40.0
SPHERE_R = 0.4  # (the camera, at 0.96 from the centre, is outside and looks at it)
# rotated, non-uniformly scaled (condition number 2), moved: the room the value must not depend on
ROOM_XF = S.translate((0.25, -0.5, 0.125)) @ S.rotate(np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0), 0.7) @ S.scale((1.0, 1.5, 0.75))
# the shading normal is the vertex normal through 10-10-10 bits (pack_normals: a component comes back up to 2^-8 low): an axis normal comes back tilted by
# delta <= sqrt(2) 2^-8 / (1 - 2^-8) against the geometric one; a transform of condition number kappa turns that into at most kappa delta
TILT = math.sqrt(2.0) * 2.0 ** -8 / (1.0 - 2.0 ** -8)


def eps(n):
    return (n + 8) * U


def f64(a):
    """the fp32 number the device holds, as float64"""
    return np.asarray(np.float32(a), np.float64)


@pytest.fixture(scope="module")
def gpu():
    from strelka_amd import build, capi

    build.build()
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def faces():
    """(centre, u, v, inward normal) of the six walls of [-1, 1]^3, u x v = the inward normal"""
    out = []
    for a in range(3):
        for s in (-1.0, 1.0):
            u, v, n = np.zeros(3), np.zeros(3), np.zeros(3)
            u[(a + 1) % 3], v[(a + 2) % 3], n[a] = 1.0, 1.0, -s
            if s > 0:
                u, v = v, u
            assert np.array_equal(np.cross(u, v), n)
            out.append((-n, u, v, n))
    return out


def quad(c, u, v):
    q = [c - u - v, c + u - v, c + u + v, c - u + v]
    return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]


def sphere_triangles(r, nu=16, nv=8):
    """a closed lat-long sphere, shared vertices bit-identical, wound outwards"""
    th, ph = np.linspace(0.0, np.pi, nv + 1), np.arange(nu) * (2 * np.pi / nu)
    P = np.float32(r * np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(nu)), np.outer(np.sin(th), np.sin(ph))], -1))
    P[0], P[nv] = np.float32([0, r, 0]), np.float32([0, -r, 0])
    tris = []
    for i in range(nv):
        for j in range(nu):
            a, b, c, d = P[i, j], P[i + 1, j], P[i + 1, (j + 1) % nu], P[i, (j + 1) % nu]
            for t in ((a, b, c), (a, c, d)):
                n = np.cross(t[1] - t[0], t[2] - t[0]).astype(np.float64)
                if np.linalg.norm(n) > 1e-9:
                    tris.append(t if n @ (t[0] + t[1] + t[2]) > 0 else (t[0], t[2], t[1]))
    assert len(tris) == 2 * nu * (nv - 1)
    return np.float32(tris)


def add_triangles(sc, tris, material, xf=None):
    t = np.asarray(tris, np.float32)
    vb, ib = S.deindex(t.reshape(-1, 3), np.arange(3 * len(t)).reshape(-1, 3))
    return sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), material, np.eye(4) if xf is None else xf)


def room(rho, instanced=False, xf=None, obj=None, light_below=False):
    """12 inward-wound triangles in one emissive MAT_DIFFUSE material (as one mesh, or as six instances of one quad mesh), the camera inside; `obj`: a white
    index-matched / ior 1.5 glass sphere of radius SPHERE_R at the centre, or a white blended card (a = 0.5, no texture) across the middle, y = 0"""
    sc = S.Scene()
    xf = np.eye(4) if xf is None else np.asarray(xf, np.float64)
    wall = sc.addMaterial(S.MAT_DIFFUSE, tuple(float(v) for v in np.broadcast_to(np.float32(rho), (3,))), emission=tuple(float(v) for v in LE))
    if instanced:
        vb, ib = S.deindex(np.float32(quad(np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))).reshape(-1, 3), np.arange(6).reshape(-1, 3))
        mesh = sc.createMesh(vb, ib)
        for c, u, v, n in faces():
            m = np.eye(4)
            m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = u, v, n, c
            sc.createInstance(S.INSTANCE_MESH, mesh, wall, xf @ m)
    else:
        add_triangles(sc, [t for c, u, v, n in faces() for t in quad(c, u, v)], wall, xf)
    if obj in ("glass10", "glass15"):
        add_triangles(sc, sphere_triangles(SPHERE_R), sc.addMaterial(S.MAT_GLASS, (1.0, 1.0, 1.0), roughness=0.0, ior=1.0 if obj == "glass10" else 1.5), xf)
    elif obj == "card":
        card = sc.addMaterial(S.MAT_DIFFUSE, (1.0, 1.0, 1.0), opacity_blend=True, opacity_scale=0.5)
        add_triangles(sc, quad(np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 0, -1.0])), card, xf)  # wound towards +Y
    else:
        assert obj is None
    if light_below:
        lx = S.translate((0.0, -1.5, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # under the floor, outside, emitting towards -Y: lights nothing, takes half the picks
        sc.createLight({"type": 0, "xform": lx, "useXform": True, "width": 1.0, "height": 0.6, "color": (10.0, 10.0, 10.0), "intensity": 1.0})
    cam = S.Camera(fov=FOV)
    cam.lookAt(tuple((xf @ [*EYE, 1.0])[:3]), tuple((xf @ [*AT, 1.0])[:3]))
    sc.addCamera(cam)
    return sc


def one_launch(ctx, sc, spp, depth, w, h, nee):
    ctx.set_option("emit_nee", nee)
    ctx.reset_stats()
    ctx.resize(w, h)
    ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=0, samples_this_launch=spp, spp_total=spp, max_depth=depth))
    img = ctx.read_accum()[..., :3].astype(np.float64)
    assert np.isfinite(img).all()
    assert (ctx.stats()["rays_shadow"] > 0) == bool(nee)
    return img


def samples_for(V, mu, target, P):
    """the smallest power of two N with 6 sqrt(V / (P N)) + eps(N) mu <= target mu in every channel"""
    N = 1
    while not (6 * np.sqrt(V / (P * N)) + eps(N) * mu <= target * mu).all():
        N *= 2
        assert P * N <= 2 ** 23, (V, mu, target)
    return N


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: deterministic -- emit_nee 0, no lights, max_depth 1 .. 5
# ---------------------------------------------------------------------------------------------------------------------------------------------
DET_W, DET_N = 8, 32


@pytest.mark.parametrize("layout", ["mesh", "instanced_top_level_transformed"])
@pytest.mark.parametrize("rho", [tuple(RHO_COLOUR), (0.5, 0.5, 0.5)], ids=["colour", "gray"])
def test_every_pixel_has_the_closed_form_up_to_depth_5(gpu, rho, layout):
    """max_depth d <= 5: no random number reaches the value, every sample of every pixel is sum_(k<d) rho^k Le (furnaceref.expected on the fp32 inputs).  Roundings of
    one sample, per channel: T_k is k products (k U), T_k Le one more, the d - 1 sums into prd.radiance U of a partial sum <= mu each: (2 d - 1) U mu in all; then
    the mean of N equal samples, eps(N) mu.  bar = (2 d + N + 8) U mu (one U for the second-order terms).
    The one way a random number does reach it: a cosine sample about the SHADING normal that falls under the GEOMETRIC horizon is absorbed (bsdf_sample's
    `dot(k2, Ng) <= 0`).  The two differ by the 10-10-10 packing's tilt delta <= TILT (kappa TILT under the room transform, kappa = 2), the sliver has the cosine-
    weighted measure delta^2 / 4 (the integral of eps d eps / pi up to delta cos(phi), over phi), and a sample absorbed at vertex k keeps what it had: it is short of
    at most mu - Le.  So a pixel may instead lie in [mu - (mu - Le) / N - bar, mu + bar] -- one absorbed sample in N --, and the pixels that need that are counted
    against lambda + 6 sqrt(lambda) + 1, lambda = pixels N d delta^2 / 4 their expected number.  Consecutive depths isolate each bounce's term: rho^d Le = mu_(d+1) - mu_d.
    `instanced_top_level_transformed`: the walls as six instances of one quad mesh, bake_world 0 (a top level), under ROOM_XF; the value depends on neither."""
    inst = layout != "mesh"
    kappa = 2.0 if inst else 1.0
    gpu.set_option("bake_world", 0 if inst else 4)
    try:
        sc = room(rho, instanced=inst, xf=ROOM_XF if inst else None)
        gpu.set_scene(sc.arrays())
        assert gpu.emitter_info()["triangles"] == 12
        prev = None
        for d in (1, 2, 3, 4, 5):
            img = one_launch(gpu, sc, DET_N, d, DET_W, DET_W, 0)
            mu = F.expected(f64(LE), f64(rho), d)
            bar = (2 * d + DET_N + 8) * U * mu
            diff = img - mu
            tight = (np.abs(diff) <= bar).all(axis=2)
            loose = ((diff <= bar) & (diff >= -(mu - f64(LE)) / DET_N - bar)).all(axis=2)
            lam = DET_W * DET_W * DET_N * d * (kappa * TILT) ** 2 / 4
            allowed = int(lam + 6 * math.sqrt(lam) + 1)
            print(f"{layout} rho {rho} depth {d}: mu {mu}, worst |diff| / bar {(np.abs(diff) / bar)[tight].max():.3f} over {int(tight.sum())} pixels, "
                  f"{int((~tight).sum())} with an absorbed sample (allowed {allowed})" + ("" if prev is None else f", term {mu - prev}"))
            assert loose.all(), (d, img[~loose], mu, bar)
            assert (~tight).sum() <= allowed
            prev = mu
    finally:
        gpu.set_option("bake_world", 4)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: deep -- max_depth 32, the roulette, NEE off and on, 1 / numPick
# ---------------------------------------------------------------------------------------------------------------------------------------------
STAT_W = 32
DEEP = [(rho, mode) for rho in (0.5, 0.8) for mode in ("nee_off", "nee_on", "nee_on_light_below")]


def deep_case(rho, mode, depth=32):
    """-> (mu_lo, mu_hi, V, N): NEE off the expectation is expected(); NEE on it is expected() + nee_reach() s_d with an s_d in [0, 1] this case does not need to know:
    nee_reach(32) = Le rho^32 g < 2e-4 mu (rho 0.8; 1e-10 mu for 0.5) widens the upper side whole"""
    nee = mode != "nee_off"
    le, r = f64(LE), f64(np.full(3, rho, np.float32))
    mu = F.expected(le, r, depth)
    hi = mu + (F.nee_reach(le, r, depth) if nee else 0.0)
    V = F.variance_bound(le, r, depth, nee, mu)
    return mu, hi, V, samples_for(V, mu, 0.01, STAT_W * STAT_W)


@pytest.mark.parametrize("rho,mode", DEEP)
def test_deep_paths_have_the_closed_form_mean(gpu, rho, mode):
    """max_depth 32, gray rho: the mean over the P = 1024 pixels and the N samples of one launch, per channel, against expected() -- the geometric series with the
    roulette's p / (p + 1e-5) per step and the rho^32 remainder left out, as the loop leaves it out.  |mean - mu| <= 6 sqrt(V / (P N)) + eps(N) mu, V
    furnaceref.variance_bound (derived from the balance heuristic and the survival probabilities, not measured); N the smallest power of two that puts the bar under
    1 % of mu.  With NEE the last vertex's share is below 2e-4 mu and widens the upper side.  `light_below`: a rect light under the floor, outside the room and
    facing away, lights nothing and takes half the picks: a wrong 1 / numPick in either technique's p_light shows.  Shadow rays exactly when NEE is on."""
    nee = mode != "nee_off"
    mu, hi, V, N = deep_case(rho, mode)
    P = STAT_W * STAT_W
    bar = 6 * np.sqrt(V / (P * N)) + eps(N) * mu
    assert (bar <= 0.01 * mu).all() and P * N <= 2 ** 23 and (hi - mu <= 2e-4 * mu).all()
    sc = room((rho,) * 3, light_below=mode == "nee_on_light_below")
    gpu.set_scene(sc.arrays())
    mean = one_launch(gpu, sc, N, 32, STAT_W, STAT_W, int(nee)).mean(axis=(0, 1))
    ratio = np.maximum(mu - mean, mean - hi) / bar
    print(f"deep rho {rho} {mode}: N {N}, mean {mean}, mu {mu}, bar / mu {bar / mu}, |diff| / bar {np.maximum(ratio, 0)}")
    assert (ratio <= 1).all(), (mean, mu, bar)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: shallow, NEE on -- one bounce's MIS weight cannot hide in the sum
# ---------------------------------------------------------------------------------------------------------------------------------------------
WALK_PATHS = 1 << 19


def shallow_case(d, frame=None):
    """-> (mu, bar, N, s_d, se): expected() + nee_reach() s_d, s_d from the float64 walk started on this camera's rays (its standard error, at 6 sigma, in the bar)"""
    sc = room(tuple(RHO_COLOUR))
    p = S.frame_params(sc.getCamera(), STAT_W, STAT_W)
    rng = np.random.default_rng(1000 + d)
    o, dirs = F.camera_rays(p["view_to_world"], p["clip_to_view"], WALK_PATHS, rng)
    le, r = f64(LE), f64(RHO_COLOUR)
    s, se, _ = F.last_vertex_share(le, r, d, o, dirs, rng)
    reach = F.nee_reach(le, r, d)
    mu = F.expected(le, r, d) + reach * s
    V = F.variance_bound(le, r, d, True, mu)
    N = samples_for(V, mu, 0.01, STAT_W * STAT_W)
    stat = 6 * np.sqrt(V / (STAT_W * STAT_W * N)) + eps(N) * mu
    return mu, stat, 6 * se * reach, N, s, se


@pytest.mark.parametrize("d", [1, 2, 3])
def test_shallow_paths_with_nee_collect_the_last_vertex_share(gpu, d):
    """max_depth 1, 2, 3 with emit_nee 1, rho = (0.3, 0.5, 0.8): the BSDF hits gather vertices 0 .. d - 1 MIS-weighted, the NEE of vertices 0 .. d - 1 the rest of
    vertices 1 .. d - 1 and the share s_d of vertex d, which no BSDF hit gathers: mu = expected() + Le rho^d s_d.  s_d is a property of the room and the camera --
    the balance-heuristic weight of the light technique, averaged over where vertex d - 1 lies -- measured by the float64 walk to its own standard error se
    (2^19 paths): bar = 6 sqrt(V / (P N)) + eps(N) mu + 6 se Le rho^d, V <= B U - mu^2 with B = (1 + rho) Le sum_(k<d) rho^k the largest sample and U = Le (sum_(k<d) rho^k + rho^d) >= mu (furnaceref.variance_bound).  N the smallest
    power of two with the statistical part under 1 % of mu.  A weight wrong at bounce d - 1 alone moves the blue channel (rho 0.8) by a multiple of that."""
    mu, stat, share, N, s, se = shallow_case(d)
    bar = stat + share
    assert 0.0 < s < 1.0 and (stat <= 0.01 * mu).all() and (share <= 0.01 * mu).all() and STAT_W * STAT_W * N <= 2 ** 23
    sc = room(tuple(RHO_COLOUR))
    gpu.set_scene(sc.arrays())
    mean = one_launch(gpu, sc, N, d, STAT_W, STAT_W, 1).mean(axis=(0, 1))
    print(f"shallow depth {d}: s_d {s:.5f} +- {se:.5f}, N {N}, mean {mean}, mu {mu}, bar / mu {bar / mu}, |diff| / bar {np.abs(mean - mu) / bar}")
    assert (np.abs(mean - mu) <= bar).all(), (mean, mu, bar)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4, 5: lossless objects in the room -- the specular protocol, fractional opacity
# ---------------------------------------------------------------------------------------------------------------------------------------------
OBJ_RHO = 0.5
OBJECTS = [("glass10", 48, 3, True), ("glass15", 48, 3, False), ("card", 32, 2, True)]  # (object, max_depth, vertices per wall vertex at worst, two-sided bracket)


def object_case(obj, depth, per_wall, two_sided, nee):
    le, r = f64(LE), f64(np.full(3, OBJ_RHO, np.float32))
    hi = F.l_inf(le, r)
    lo = hi * (1.0 - r ** (depth // per_wall)) if two_sided else np.zeros(3)
    V = F.variance_bound_objects(le, r, nee, lo)
    N = samples_for(V, hi, 0.02, STAT_W * STAT_W)
    return lo, hi, 6 * np.sqrt(V / (STAT_W * STAT_W * N)) + eps(N) * hi, N


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("obj,depth,per_wall,two_sided", OBJECTS)
def test_lossless_objects_leave_the_furnace_unchanged(gpu, obj, depth, per_wall, two_sided, nee):
    """A white lossless object in the room changes no radiance: the mean stays the full series L_inf = Le / (1 - rho) less what the depth limit cuts off.
      glass10: a tessellated white MAT_GLASS sphere, smooth, ior 1.0.  Fresnel is zero, every encounter is two specular transmissions and the path goes straight
        on.  The sphere is convex: of three consecutive vertices at most two are glass, a path of d = 48 vertices has >= 16 wall vertices:
        mean in [L_inf (1 - rho^16), L_inf].  NEE taken at a specular vertex, an MIS-weighted emitter hit after a specular bounce (lastBsdfPdf = 1 makes the weight
        1 / (1 + p_light): tens of percent), an `inside` flag that does not come back (the walls would then be shaded from behind) and an offset_ray to the wrong
        side (the path meets the face it left again) all leave that bracket.
      glass15: the same sphere with ior 1.5 reflects, refracts and totally reflects; a lossless object creates no energy: mean <= L_inf.  ONE-SIDED: inside the
        sphere a path can be reflected any number of times, so no fixed number of wall vertices -- and no lower side below the bar -- follows from d.
      card: a white non-emitting MAT_DIFFUSE card, blended with a = 0.5 (opacity_scale 0.5, no texture), across the middle of the room.  The stochastic
        pass-through of radiance rays (probability 1 - a) and the factor 1 - a of the shadow rays that cross it have to agree for L_inf to survive.  d = 32.
        (A card hit from behind takes no NEE sample -- the light sample is tested against the unflipped shading normal, the reference's two-sided convention --
        and leaves along offset_ray's front side, so it meets the card once more: the premise "every other vertex a wall" is "every third" at worst, rho^10 instead
        of rho^16 and still 1e-3 of L_inf, a twentieth of the bar; measured with NEE: 0.34 % under L_inf.)
    The roulette's p / (p + 1e-5) takes at most 3.2e-4 + 47 * 2e-5 = 1.3e-3 of L_inf here (p = rho^j >= rho^5 at the first step, >= 0.4998 later): far inside the
    bar.  bar = 6 sqrt(V / (P N)) + eps(N) L_inf, V furnaceref.variance_bound_objects (walls and objects in any order); N the smallest power of two with the bar
    under 2 % of L_inf -- what this case exists to catch moves the mean by the NEE's share of a vertex, several bars."""
    lo, hi, bar, N = object_case(obj, depth, per_wall, two_sided, bool(nee))
    assert (bar <= 0.02 * hi).all() and STAT_W * STAT_W * N <= 2 ** 23
    sc = room((OBJ_RHO,) * 3, obj=obj)
    gpu.set_scene(sc.arrays())
    mean = one_launch(gpu, sc, N, depth, STAT_W, STAT_W, nee).mean(axis=(0, 1))
    ratio = np.maximum(lo - mean, mean - hi) / bar
    print(f"{obj} emit_nee {nee}: N {N}, mean {mean}, bracket [{lo}, {hi}], bar / L_inf {bar / hi}, outside by / bar {np.maximum(ratio, 0)}, (mean - L_inf) / bar {(mean - hi) / bar}")
    if obj == "card":
        bi = gpu.blend_info()
        assert bi["active_materials"] == 1 and bi["passed_radiance"] > 0 and (bi["crossed_shadow"] > 0) == bool(nee) and bi["accepted_by_cap"] == 0
    assert (ratio <= 1).all(), (mean, lo, hi, bar)


def pixels_through_the_sphere(sc, w, h):
    """pixels whose four corner rays (generate_camera_ray in float64) all pass within 0.9 SPHERE_R of the centre: the tessellated sphere's faces lie beyond
    cos(pi / 16)^2 = 0.96 of its radius, so every sample of such a pixel enters it"""
    p = S.frame_params(sc.getCamera(), w, h)
    V, C = np.asarray(p["view_to_world"], np.float64).reshape(4, 4), np.asarray(p["clip_to_view"], np.float64).reshape(4, 4)
    gx, gy = np.meshgrid(np.arange(w + 1) / w * 2 - 1, np.arange(h + 1) / h * 2 - 1)
    vs = np.stack([gx, gy, np.ones_like(gx), np.ones_like(gx)], -1) @ C.T
    vs[..., 3] = 0.0
    d = (vs @ V.T)[..., :3]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    near = np.linalg.norm(np.cross(np.broadcast_to(V[:3, 3], d.shape), d), axis=-1) <= 0.9 * SPHERE_R
    return near[:-1, :-1] & near[1:, :-1] & near[:-1, 1:] & near[1:, 1:]


def test_behind_the_index_matched_sphere_every_sample_carries_the_full_emission(gpu):
    """The specular protocol sample by sample: ONE sample per pixel, max_depth 3, the pixels whose rays enter the ior 1.0 sphere.  Vertices 0 and 1 are specular
    transmissions with bsdf_over_pdf = base = 1, vertex 2 is a wall met after a specular bounce: it adds T Le = Le at full weight, exactly -- no rounding, T is 1.
    emit_nee 0: the pixel IS Le, bit for bit.  emit_nee 1: vertex 2's NEE adds something >= 0 on top: every pixel >= Le, most above it.  An emitter hit that is
    MIS-weighted after a specular bounce returns Le / (1 + p_light) and falls below wherever the light sample is invalid (a sixth of them lie on the wall itself);
    NEE at a glass vertex, a path that does not leave the sphere or leaves it with `inside` set, shows in the emit_nee 0 image."""
    sc = room(tuple(RHO_COLOUR), obj="glass10")
    gpu.set_scene(sc.arrays())
    sel = pixels_through_the_sphere(sc, STAT_W, STAT_W)
    assert sel.sum() >= 200
    off = one_launch(gpu, sc, 1, 3, STAT_W, STAT_W, 0)
    on = one_launch(gpu, sc, 1, 3, STAT_W, STAT_W, 1)
    le = f64(LE)
    print(f"{int(sel.sum())} pixels through the sphere: emit_nee 0 max |pixel - Le| {np.abs(off[sel] - le).max():.3e}, emit_nee 1 min (pixel - Le) {(on[sel] - le).min():.3e}, "
          f"above Le {(on[sel] > le).all(axis=1).mean():.3f}")
    assert np.array_equal(off[sel], np.broadcast_to(le, off[sel].shape))
    assert (on[sel] >= le).all() and (on[sel] > le).all(axis=1).mean() > 0.5
