"""Emissive meshes on the GPU ("Emissive meshes").  The CPU checker knows no emission, so nothing here is "HIP == oracle": the
emitter table and the device functions are held against the float64 restatement in tests/emitref.py through skh_emitter_probe (which calls the
`__device__` functions k_shade calls), the integrator against Lambert's polygon formula with bounds DERIVED from the scene.

U = 2^-24 is half an ulp, relative.  The scenes of the table tests keep every WORLD-space vertex an exact fp32 number with exact differences (grid
coordinates, power-of-two scales): what separates the device's table from float64 is then the evaluation of area * luminance alone, bounded per entry by
emitref.weight_error_bound; the sums are doubles on both sides (error ~ N 2^-53, not counted)."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes, tiles
from tests import emitref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


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


def add_triangles(sc, tris, material, xf=None):
    """tris: (N, 3, 3) object-space vertices; triangle k of the mesh is tris[k], vertex order kept"""
    t = np.asarray(tris, np.float32)
    vb, ib = S.deindex(t.reshape(-1, 3), np.arange(3 * len(t)).reshape(-1, 3))
    return sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), material, np.eye(4) if xf is None else xf)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the two table scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
FAN_LE = (np.float32([4.0, 2.0, 1.0]), np.float32([0.5, 3.0, 6.0]))
FAN_XF = S.translate((0.5, 1.0, -0.25)) @ S.scale((2.0, 1.0, 0.5))  # non-uniform, powers of two: exact in fp32
FAN_MIRROR = S.translate((8.0, 0.0, 0.0)) @ S.scale((-1.0, 1.0, 1.0))


def fan_triangles():
    """300 triangles around the origin in the plane y = 0, rim radii 1 ... 2 and uneven angles, every coordinate a multiple of 2^-10"""
    rs = np.random.RandomState(17)
    ang = np.cumsum(0.5 + rs.rand(300))
    ang = ang / ang[-1] * 2 * np.pi
    ang = np.concatenate([[0.0], ang[:-1], [0.0]])  # closed
    r = 1.0 + rs.rand(301)
    r[-1] = r[0]
    rim = np.round(np.stack([r * np.cos(ang), np.zeros(301), r * np.sin(ang)], 1) * 1024) / 1024
    tris = np.zeros((300, 3, 3))
    tris[:, 1], tris[:, 2] = rim[:-1], rim[1:]
    return tris.astype(np.float32)


def fan_scene(mirror=False):
    """the fan as two instances of 150 triangles with two emissive materials (+ a mirrored third instance of the first half, + a mesh that does not emit)"""
    sc = S.Scene()
    grey = sc.addMaterial(S.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    mats = [sc.addMaterial(S.MAT_DIFFUSE, (0.2, 0.2, 0.2), emission=tuple(float(v) for v in le)) for le in FAN_LE]
    t = fan_triangles()
    add_triangles(sc, t[:7] + np.float32([0, -3, 0]), grey)  # instance 0: not an emitter
    inst = [add_triangles(sc, t[:150], mats[0], FAN_XF), add_triangles(sc, t[150:], mats[1], FAN_XF)]
    world = [emitref.world_triangles(t[:150], FAN_XF), emitref.world_triangles(t[150:], FAN_XF)]
    les = [FAN_LE[0], FAN_LE[1]]
    flips = [False, False]
    if mirror:
        inst.append(add_triangles(sc, t[:150], mats[1], FAN_MIRROR))
        world.append(emitref.world_triangles(t[:150], FAN_MIRROR))
        les.append(FAN_LE[1]), flips.append(True)
    cam = S.Camera(fov=40.0)
    cam.lookAt((0.0, 6.0, 0.1), (0.0, 0.0, 0.0))
    sc.addCamera(cam)
    return sc, table_of(inst, world, les, flips)


def table_of(inst, world, les, flips):
    n = [len(w) for w in world]
    t = {"world": np.concatenate(world), "Le": np.concatenate([np.broadcast_to(le, (k, 3)) for le, k in zip(les, n)]),
         "instance": np.concatenate([np.full(k, i) for i, k in zip(inst, n)]), "prim": np.concatenate([np.arange(k) for k in n]),
         "flip": np.concatenate([np.full(k, f) for f, k in zip(flips, n)]), "base": dict(zip(inst, np.cumsum([0] + n[:-1])))}
    t["lum"] = emitref.lum709(t["Le"])
    t["w"], t["cdf"], t["sum_w"] = emitref.table(t["world"], t["lum"])
    assert (t["world"].astype(np.float32) == t["world"]).all()  # the premise of the bars: world-space vertices that fp32 holds exactly
    return t


GRID_LE = np.float32([3.0, 2.0, 1.0])


def grid_scene():
    """a 1.0 x 0.5625 quad at height 1.5 facing down as 256 x 144 cells = 73 728 triangles (> 256 x 256: the scan crosses workgroups and its single-workgroup
    pass sees 36 tiles), interior vertices jittered by up to 2/16 of a cell in x and z (no triangle can flip: its doubled area stays >= 12 * 12 - 4 * 20 > 0
    sixteenths squared; the areas spread over 1 : 3); coordinates multiples of 2^-12"""
    nx, nz = 256, 144
    rs = np.random.RandomState(5)
    gx, gz = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
    x, z = gx * 16.0, gz * 16.0  # in units of 2^-12
    inner = (gx > 0) & (gx < nx) & (gz > 0) & (gz < nz)
    x = x + np.where(inner, rs.randint(-2, 3, x.shape), 0)
    z = z + np.where(inner, rs.randint(-2, 3, z.shape), 0)
    P = np.stack([x / 4096.0 - 0.5, np.full(x.shape, 1.5), z / 4096.0 - 0.28125], -1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.stack([np.stack([a, b, c], 2), np.stack([a, c, d], 2)], 2).reshape(-1, 3, 3)  # (x, z) winding: the normal points to -Y
    sc = S.Scene()
    m = sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0), emission=tuple(float(v) for v in GRID_LE))
    i = add_triangles(sc, tris, m)
    cam = S.Camera(fov=40.0)
    cam.lookAt((0.0, 0.2, 0.0), (0.0, 1.5, 0.01))
    sc.addCamera(cam)
    return sc, table_of([i], [emitref.world_triangles(tris.astype(np.float32))], [GRID_LE], [False])


@pytest.fixture(scope="module")
def fan(gpu):
    sc, t = fan_scene()
    return sc, t


@pytest.fixture(scope="module")
def grid():
    return grid_scene()


def sample(c, t, u, ux, uy, P):
    rec = np.zeros((len(u), 6), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3:6] = u, ux, uy, P
    o = c.emitter_probe("sample", rec)
    s = {"point": f32(o[:, 0:3]), "normal": f32(o[:, 3:6]), "Le": f32(o[:, 6:9]), "pdf": f32(o[:, 9:10])[:, 0], "dist": f32(o[:, 10:11])[:, 0],
         "instance": o[:, 11].astype(np.int64), "prim": o[:, 12].astype(np.int64)}
    base = np.full(max(t["base"]) + 1, -1, np.int64)
    for i, b in t["base"].items():
        base[i] = b
    assert (s["instance"] <= max(t["base"])).all() and (base[s["instance"]] >= 0).all()  # every sample names an emitting instance
    s["entry"] = base[s["instance"]] + s["prim"]
    return s


def pdf_probe(c, instance, prim, x, origin):
    rec = np.zeros((len(instance), 8), np.uint32)
    rec[:, 0], rec[:, 1] = instance, prim
    rec[:, 2:5], rec[:, 5:8] = np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(origin, np.float32).view(np.uint32)
    o = c.emitter_probe("pdf", rec)
    return f32(o[:, 0:1])[:, 0], f32(o[:, 1:4])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the table and the selection
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fan", "grid"])
def test_table_against_float64(gpu, fan, grid, which):
    """sum w against the float64 sum of the same fp32 inputs.  The bar: every stored weight is off by at most emitref.weight_error_bound (the fp32 cross
    product, length, two products: derived there, ~ (|e1|_1 |e2|_1 / |e1 x e2| + 10) U relative -- a sliver of the fan pays 1 / sin of its angle), the
    sum of N floats in double adds N 2^-53: bar = sum of the per-entry bounds / sum w."""
    sc, t = fan if which == "fan" else grid
    gpu.set_scene(sc.arrays(), build=False)  # (the table needs no acceleration structure)
    info = gpu.emitter_info()
    n = len(t["w"])
    assert info["triangles"] == n and info["instances"] == len(t["base"]) and n == (300 if which == "fan" else 73728)
    bar = float(emitref.weight_error_bound(t["world"], t["lum"]).sum() / t["sum_w"]) + n * 2.0 ** -53
    rel = abs(info["sum_w"] / t["sum_w"] - 1)
    print(f"{which}: {n} entries, sum w {info['sum_w']!r} against {t['sum_w']!r}: relative {rel:.3e} (bar {bar:.3e}), {info['bytes']} B, built in {info['ms_build']:.3f} ms")
    assert rel <= bar
    assert 64 * n + 4 * n < info["bytes"] <= 76 * n + 4096  # 64 B entries + 4 B CDF + a guide of at most 2 n + 1 words + the per-material / per-instance words


@pytest.mark.parametrize("which", ["fan", "grid"])
def test_selection_follows_the_cdf(gpu, fan, grid, which):
    """u'_j = (j + 1/2) / 2^20, every one exact in fp32.  Entries k0 <= k < k1 are selected by the u' in [CDF(k0), CDF(k1)): 2^20 (CDF64(k1) - CDF64(k0))
    of the grid points, within +-4: a threshold one float rounding from exact moves an end by <= 2^-25 < one grid step, the stored weights' relative error
    (~1e-6) moves it by about one grid point: +-2 per end.  On the fan the selected entry must be emitref's wherever u' is further than 2^-20 from a boundary."""
    sc, t = fan if which == "fan" else grid
    gpu.set_scene(sc.arrays(), build=False)
    M = 1 << 20
    u = ((np.arange(M) + 0.5) / M).astype(np.float32)
    assert (u.astype(np.float64) * M - 0.5 == np.arange(M)).all()
    s = sample(gpu, t, u, np.full(M, 0.5, np.float32), np.full(M, 0.5, np.float32), np.zeros((M, 3), np.float32))
    n = len(t["w"])
    assert (s["entry"] < n).all() and (np.diff(s["entry"]) >= 0).all()  # monotone in u'
    counts = np.bincount(s["entry"], minlength=n)
    cdf0 = np.concatenate([[0.0], t["cdf"]])
    worst = 0.0
    for k0 in range(0, n, 1024):
        k1 = min(k0 + 1024, n)
        want = M * (cdf0[k1] - cdf0[k0])
        worst = max(worst, abs(counts[k0:k1].sum() - want))
    print(f"{which}: bins of 1024 entries, worst |count - 2^20 dCDF| = {worst:.2f}")
    assert worst <= 4
    assert (t["w"][s["entry"]] > 0).all()
    if which == "fan":
        ref = emitref.select(t["cdf"], u)
        d = np.minimum(np.abs(u - cdf0[ref]), np.abs(cdf0[ref + 1] - u))
        clear = d > 2.0 ** -20
        print(f"fan: {1 - clear.mean():.4%} of the draws within 2^-20 of a boundary; mismatches among the others {int((s['entry'][clear] != ref[clear]).sum())}")
        assert 1 - clear.mean() <= 0.01
        assert np.array_equal(s["entry"][clear], ref[clear])


def test_a_single_triangle_and_the_ends_of_the_draw(ctx):
    sc = S.Scene()
    m = sc.addMaterial(S.MAT_DIFFUSE, (0, 0, 0), emission=(1.0, 1.0, 1.0))
    i = add_triangles(sc, np.float32([[(0, 2, 0), (1, 2, 0), (0, 2, 1)]]), m)
    ctx.set_scene(sc.arrays(), build=False)
    info = ctx.emitter_info()
    assert info["triangles"] == 1 and info["instances"] == 1 and abs(info["sum_w"] - 0.5 * float(np.float32(emitref.lum709(np.ones(3))))) <= 4 * U
    t = table_of([i], [emitref.world_triangles(np.float32([[(0, 2, 0), (1, 2, 0), (0, 2, 1)]]))], [np.ones(3, np.float32)], [False])
    u = np.float32([0.0, 0.5, 0.99999994, 1.0, 2.0, -1.0, np.nan])
    s = sample(ctx, t, u, np.full(7, 0.25, np.float32), np.full(7, 0.5, np.float32), np.zeros((7, 3), np.float32))
    assert (s["entry"] == 0).all() and np.array_equal(s["point"], np.broadcast_to(np.float32([0.25, 2, 0.25]), (7, 3)))
    assert np.array_equal(s["normal"], np.broadcast_to(np.float32([0, -1, 0]), (7, 3)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: probe values
# ---------------------------------------------------------------------------------------------------------------------------------------------
def normal_fp32(world, flip):
    """emit_normal restated in numpy fp32, operation by operation (-ffp-contract=off: the device rounds the same way)"""
    v = world.astype(np.float32)
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    inv = np.float32(1.0) / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    n = c * inv[:, None]
    return np.where(flip[:, None], -n, n)


def test_probe_values(ctx):
    """point: every barycentric weight carries <= 3 U absolute (sqrt, 1 - su, 1 - uy, one product), the three products and two sums per coordinate 4 U more:
    |point - emitref.point| <= 12 U max|v| per coordinate, and so is its distance from the plane (x sqrt 3).  normal: bit-equal to the fp32 restatement,
    within 4 U of float64 here (the fan lies in a coordinate plane).  Le: the caller's bits.  pdf = (lum / sum w) dist^2 / cos_e at the RETURNED point:
    relative error <= e_sum (test_table_against_float64's bar) + 3 U (luminance, reciprocal of sum w, their product) + 9 U (dist^2: a difference, three
    squares, two sums, a root, a square) + 2 U (the product and the quotient) + (8 + kappa) U / cos_e (the unit direction: 5 U; the dot product: 3 U of
    sum |L_i n_i| <= 1; the normal: kappa = |e1|_1 |e2|_1 / |e1 x e2| + 4), all of it relative to the cosine."""
    sc, t = fan_scene(mirror=True)
    ctx.set_scene(sc.arrays(), build=False)
    info = ctx.emitter_info()
    n = len(t["w"])
    assert info["triangles"] == n == 450
    e_sum = float(emitref.weight_error_bound(t["world"], t["lum"]).sum() / t["sum_w"]) + n * 2.0 ** -53
    rs = np.random.RandomState(23)
    m = 200000
    u, ux, uy = (rs.rand(m).astype(np.float32) for _ in range(3))
    P = (rs.rand(m, 3) * [12, 4, 8] - [3, 5, 4]).astype(np.float32)  # below the fans, which emit towards -Y
    P[: m // 4, 1] += 6.0  # a quarter of them ABOVE: behind the emitters
    s = sample(ctx, t, u, ux, uy, P)
    k = s["entry"]
    tri = t["world"][k]
    assert np.array_equal(s["instance"], t["instance"][k]) and np.array_equal(s["prim"], t["prim"][k])
    vmax = np.abs(tri).max(axis=(1, 2))
    want_pt = emitref.point(tri, ux, uy)
    err = np.abs(s["point"] - want_pt).max(axis=1) / vmax
    n64 = emitref.normal(tri)
    n64 = np.where(t["flip"][k][:, None], -n64, n64)
    plane = np.abs(((s["point"].astype(np.float64) - tri[:, 0]) * n64).sum(1)) / vmax
    print(f"point: max |diff| / max|v| = {err.max() / U:.2f} U (bar 12 U), off the plane {plane.max() / U:.2f} U (bar {12 * math.sqrt(3):.1f} U)")
    assert (err <= 12 * U).all() and (plane <= 12 * math.sqrt(3) * U).all()
    assert np.array_equal(s["normal"].view(np.uint32), normal_fp32(tri, t["flip"][k]).astype(np.float32).view(np.uint32))
    assert np.abs(s["normal"] - n64).max() <= 4 * U
    assert np.array_equal(s["Le"].view(np.uint32), t["Le"][k].astype(np.float32).view(np.uint32))
    # the emitting side: the fan's winding (0, rim_i, rim_i+1) with growing angle in (x, z) points to -Y; the mirrored instance keeps that side
    assert (n64[:, 1] < 0).all()
    d = s["point"].astype(np.float64) - P
    dist = np.linalg.norm(d, axis=1)
    assert (np.abs(s["dist"] / dist - 1) <= 5 * U).all()
    want = emitref.pdf(n64, t["lum"][k], t["sum_w"], s["point"].astype(np.float64), P.astype(np.float64))
    cos_e = -(d * n64).sum(1) / dist
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    kappa = np.abs(e1).sum(1) * np.abs(e2).sum(1) / np.linalg.norm(np.cross(e1, e2), axis=1) + 4
    front = cos_e > 1e-3
    bar = e_sum + 14 * U + (8 + kappa) * U / np.where(front, cos_e, 1.0)
    rel = np.abs(s["pdf"].astype(np.float64) - want) / np.where(front, want, 1.0)
    print(f"pdf: max relative error / bar = {(rel[front] / bar[front]).max():.3f} over {int(front.sum())} front-side samples; {int((cos_e < -1e-3).sum())} from behind")
    assert (rel[front] <= bar[front]).all()
    assert (s["pdf"][cos_e < -1e-3] == 0).all() and (cos_e < -1e-3).sum() > m // 8  # a point behind the emitter gets pdf 0
    # the PDF probe at the sampled point: the same function, the same bits; Le too
    pp, ple = pdf_probe(ctx, s["instance"], s["prim"], s["point"], P)
    assert np.array_equal(pp.view(np.uint32), s["pdf"].view(np.uint32)) and np.array_equal(ple.view(np.uint32), s["Le"].view(np.uint32))
    # ... and zeros for a triangle that is not in the table: a mesh that does not emit, a primitive past the instance's end, an instance that does not exist
    z, zle = pdf_probe(ctx, np.array([0, 1, 99]), np.array([0, 150, 0]), np.float32([[0, 0, 0]] * 3), np.float32([[0, -1, 0]] * 3))
    assert (z == 0).all() and (zle == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: the closed form
# ---------------------------------------------------------------------------------------------------------------------------------------------
RHO = 0.5
QUAD = np.array([(-0.5, 1.5, -0.3), (0.5, 1.5, -0.3), (0.5, 1.5, 0.3), (-0.5, 1.5, 0.3)])  # 1.0 x 0.6 at height 1.5; this order winds towards -Y
LE = np.float32([10.0, 6.0, 3.0])


def quad_triangles(nx=1, nz=1, flip=False):
    gx, gz = np.meshgrid(np.arange(nx + 1) / nx - 0.5, (np.arange(nz + 1) / nz - 0.5) * 0.6, indexing="ij")
    P = np.stack([gx, np.full(gx.shape, 1.5), gz], -1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    t = np.stack([np.stack([a, b, c], 2), np.stack([a, c, d], 2)], 2).reshape(-1, 3, 3)
    return t[:, ::-1].copy() if flip else t


def lit_floor(cam_from, cam_at, tess=False, light_below=False, le=LE, up=False, base=(0.0, 0.0, 0.0), blocker=False):
    """the floor, material, camera style and 8 x 8 launch of tests/test_gpu_env.py::floor_scene, under a black emissive 1.0 x 0.6 quad at height 1.5"""
    sc = S.Scene()
    grey = sc.addMaterial(S.MAT_DIFFUSE, (RHO, RHO, RHO))
    lamp = sc.addMaterial(S.MAT_DIFFUSE, base, emission=None if le is None else tuple(float(v) for v in le))
    add_triangles(sc, np.float32([[(-20, 0, 20), (20, 0, 20), (20, 0, -20)], [(-20, 0, 20), (20, 0, -20), (-20, 0, -20)]]), grey)
    e = add_triangles(sc, quad_triangles(16, 10, up) if tess else quad_triangles(1, 1, up), lamp)
    if blocker:
        # (small enough for the camera to look past it, large enough to hide the whole quad from the floor the pixels see)
        add_triangles(sc, np.float32([[(-1.2, 0.75, 1.2), (1.2, 0.75, 1.2), (1.2, 0.75, -1.2)], [(-1.2, 0.75, 1.2), (1.2, 0.75, -1.2), (-1.2, 0.75, -1.2)]]), grey)
    if light_below:
        xf = S.translate((0.0, -1.5, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # emits towards -Y, away from the floor above it
        sc.createLight({"type": 0, "xform": xf, "useXform": True, "width": 1.0, "height": 0.6, "color": (10.0, 10.0, 10.0), "intensity": 1.0})
    cam = S.Camera(fov=1.5)
    cam.lookAt(cam_from, cam_at)
    sc.addCamera(cam)
    return sc, e


def one_launch(ctx, sc, spp, depth, w=8, h=8, **kw):
    ctx.resize(w, h)
    ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=0, samples_this_launch=spp, spp_total=spp, max_depth=depth, **kw))
    return ctx.read_accum()[..., :3].astype(np.float64)


def floor_points(sc, w, h):
    """where the rays through the pixels' centres and corners meet the floor y = 0: (h, w, 5, 3), generate_camera_ray in float64"""
    p = S.frame_params(sc.getCamera(), w, h)
    V, Cm = np.asarray(p["view_to_world"], np.float64).reshape(4, 4), np.asarray(p["clip_to_view"], np.float64).reshape(4, 4)
    out = np.zeros((h, w, 5, 3))
    o = (V @ [0, 0, 0, 1])[:3]
    for py in range(h):
        for px in range(w):
            for k, (jx, jy) in enumerate(((0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1))):
                ndc = np.array([(px + jx) / w * 2 - 1, (py + jy) / h * 2 - 1, 1.0, 1.0])
                vs = Cm @ ndc
                d = (V @ [vs[0], vs[1], vs[2], 0.0])[:3]
                out[py, px, k] = o + d * (-o[1] / d[1])
    return out


VIEWS = {"under": ((3.0, 1.0, 0.4), (0.0, 0.0, 0.0)), "off_axis": ((5.0, 1.0, 1.4), (2.0, 0.0, 1.0))}


# (quad as 2 triangles / 320) x (view) x (depth 2 / 4), and once more per view with a rect light under the floor
CLOSED_FORM_CASES = [(t, v, d, False) for t in (False, True) for v in ("under", "off_axis") for d in (2, 4)] + [(False, "under", 2, True), (False, "off_axis", 2, True)]


@pytest.mark.parametrize("tess,view,depth,light_below", CLOSED_FORM_CASES)
def test_floor_under_an_emissive_quad_has_its_closed_form(ctx, tess, view, depth, light_below):
    """A floor point p sees the quad and nothing it reflects comes back (the quad is black, the floor flat): a pixel's expectation is rho Le E(p) / pi, E / Le
    Lambert's polygon formula.  One launch of N samples, the mean over the P = 64 pixels, per channel: |mean - mu| <= 6 sqrt(V / (P N)) + eps(N) mu + spread.
      emit_nee 0: a sample is rho Le or 0 -> V = mu (rho Le - mu);   emit_nee 1: each technique's weighted sample is <= rho Le by the balance heuristic, their
      sum in [0, 2 rho Le] -> V <= mu (2 rho Le - mu) (Bhatia-Davis).   spread: the formula at the pixel's corners against its centre.
    N is the smallest power of two that puts the bound below 10 % of mu: 2 048 under the quad (8.5 %); 32 768 -- P N = 2 10^6 paths -- for the off-axis view (8.7 %, 2.2 % of
    it the spread: the 8 x 8 pixels cover 22 cm of floor), where cos_e = 0.56 -- a stray or a missing cosine is a 44 % error --; a
    rect light UNDER the floor lights nothing and takes half the picks: a wrong 1 / numPick shows.  The emitter must not shadow itself: that halves emit_nee 1."""
    N, Pn = {"under": 2048, "off_axis": 32768}[view], 64
    sc, _ = lit_floor(*VIEWS[view], tess=tess, light_below=light_below)
    ctx.set_scene(sc.arrays())
    fpts = floor_points(sc, 8, 8)
    E = np.array([[[emitref.polygon_irradiance(QUAD, fpts[y, x, k], (0, 1, 0)) for k in range(5)] for x in range(8)] for y in range(8)])
    if view == "off_axis":
        d = np.array([0, 1.5, 0]) - fpts[:, :, 0].reshape(-1, 3).mean(0)
        assert abs(d[1] / np.linalg.norm(d) - 0.56) < 0.01
    rl = RHO * LE.astype(np.float64)
    mu_px = E[:, :, 0, None] * rl / np.pi  # (8, 8, 3)
    mu = mu_px.mean(axis=(0, 1))
    spread = np.abs(E[:, :, 1:] - E[:, :, :1]).max(axis=2).mean() * rl / np.pi
    mse = {}
    for nee in (0, 1):
        ctx.set_option("emit_nee", nee)
        ctx.reset_stats()
        img = one_launch(ctx, sc, N, depth)
        mean = img.mean(axis=(0, 1))
        V = mu * ((2 if nee else 1) * rl - mu)
        bound = 6 * np.sqrt(V / (Pn * N)) + eps(N) * mu + spread
        mse[nee] = float(((img - mu_px) ** 2).mean())
        print(f"tess {tess} {view} depth {depth} below {light_below} emit_nee {nee}: mean {mean}, mu {mu}, |diff| / bound {np.abs(mean - mu) / bound}, "
              f"bound / mu {bound / mu}, per-pixel MSE {mse[nee]:.4e}, shadow rays {ctx.stats()['rays_shadow']}")
        assert (bound <= 0.1 * mu).all()
        assert (np.abs(mean - mu) <= bound).all(), (nee, mean, mu, bound)
        assert (ctx.stats()["rays_shadow"] > 0) == bool(nee)  # (a sample of the light under the floor is below the horizon: no ray)
    assert mse[1] < mse[0], mse


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: occlusion and sides
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_occlusion_and_sides(ctx):
    # an opaque quad between emitter and floor: nothing arrives, and the shadow rays that say so were traced
    sc, _ = lit_floor(*VIEWS["under"], blocker=True)
    ctx.set_scene(sc.arrays())
    ctx.reset_stats()
    img = one_launch(ctx, sc, 256, 1)
    assert (img == 0).all() and ctx.stats()["rays_shadow"] > 0
    # an emitter that faces up, away from the floor, lights nothing: no valid sample (no shadow ray), and a BSDF ray reaches its back
    sc, _ = lit_floor(*VIEWS["under"], up=True)
    ctx.set_scene(sc.arrays())
    for nee in (1, 0):
        ctx.set_option("emit_nee", nee)
        ctx.reset_stats()
        assert (one_launch(ctx, sc, 256, 3) == 0).all() and ctx.stats()["rays_shadow"] == 0
    ctx.set_option("emit_nee", 1)
    # a camera that looks at the front sees Le exactly: throughput 1, weight 1 at depth 0, then the accumulate step's known arithmetic
    sc, _ = lit_floor((0.0, 0.2, 0.0), (0.05, 1.5, 0.02))
    ctx.set_scene(sc.arrays())
    n = 5
    ctx.resize(16, 16)
    for i in range(n):
        ctx.render_subframe(S.frame_params(sc.getCamera(), 16, 16, subframe_index=i, spp_total=n, max_depth=4))
    img = ctx.read_accum()[..., :3]
    e = S.default_exposure()
    want = f32(ctx.unit_probe("accumulate", np.broadcast_to(LE, (n, 3)).copy(), param=0, consts=np.ascontiguousarray(e, np.float32)))[n - 1]
    assert np.array_equal(img.view(np.uint32), np.broadcast_to(want, img.shape).copy().view(np.uint32))


def test_the_back_of_an_emitter_is_an_ordinary_surface(ctx):
    """a grey emissive quad facing down, seen from above under a rect light: with emit_nee 0 the pick is the light alone, the back emits nothing, and every
    operation on the path is the one a context without emission performs -- the same bits.  (max_depth 1: primary hits and their light samples; a
    bounce off the floor would reach the quad's FRONT, which does emit)"""
    from strelka_amd import capi

    def scene(le):
        sc, _ = lit_floor((0.3, 4.0, 0.2), (0.0, 1.5, 0.0), le=le, base=(0.6, 0.5, 0.4))
        xf = S.translate((1.5, 3.0, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # beside the camera's line of sight, emitting downwards
        sc.createLight({"type": 0, "xform": xf, "useXform": True, "width": 1.0, "height": 1.0, "color": (10.0, 10.0, 10.0), "intensity": 1.0})
        sc.getCamera().fov = 20.0
        return sc

    sc = scene(LE)
    ctx.set_scene(sc.arrays())
    assert ctx.emitter_info()["triangles"] == 2
    ctx.set_option("emit_nee", 0)
    a = one_launch(ctx, sc, 64, 1, 16, 16)
    plain = capi.Context(0)
    try:
        sc0 = scene(None)
        plain.set_scene(sc0.arrays())
        b = one_launch(plain, sc0, 64, 1, 16, 16)
    finally:
        plain.close()
    assert a.max() > 0 and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: nothing changes without emission
# ---------------------------------------------------------------------------------------------------------------------------------------------
def render(ctx, sc, w, h, n, depth=4, **kw):
    ctx.resize(w, h)
    for i in range(n):
        ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=n, max_depth=depth, **kw))
    return ctx.read_accum()[..., :3].copy()


def test_nothing_changes_without_emission(ctx):
    from strelka_amd import capi

    sc = scenes.cornell_box()
    arr = sc.arrays()
    never = capi.Context(0)
    try:
        never.set_scene(arr)
        want = render(never, sc, 48, 48, 4)
    finally:
        never.close()
    ctx.set_scene(arr)
    nm = len(arr["materials"])
    ctx.set_emission(np.zeros((nm, 3), np.float32))
    assert ctx.emitter_info()["triangles"] == 0
    assert np.array_equal(render(ctx, sc, 48, 48, 4), want)
    em = np.zeros((nm, 3), np.float32)
    em[0] = (2.0, 2.0, 2.0)
    ctx.set_emission(em)
    assert ctx.emitter_info()["triangles"] > 0
    lit = render(ctx, sc, 48, 48, 4)
    assert not np.array_equal(lit, want) and np.isfinite(lit).all()
    ctx.set_emission(None)
    info = ctx.emitter_info()
    assert info["triangles"] == 0 and info["bytes"] == 0 and info["sum_w"] == 0
    assert np.array_equal(render(ctx, sc, 48, 48, 4), want)
    ctx.set_option("emit_nee", 0)  # with no emissive material the option changes nothing
    assert np.array_equal(render(ctx, sc, 48, 48, 4), want)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: staleness
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fresh_image(arr, sc, **kw):
    from strelka_amd import capi

    c = capi.Context(0)
    try:
        c.set_scene(arr)
        return render(c, sc, 32, 32, 3, **kw)
    finally:
        c.close()


def test_the_table_follows_the_scene(ctx):
    """each edit through the path an application takes; the image equals the one of a fresh context given the edited scene (the hierarchy after an update
    returns the hits of a rebuild: tests/test_gpu_update.py)"""
    sc, e = lit_floor((2.0, 1.2, 1.5), (0.0, 0.0, 0.0), tess=True)
    sc.getCamera().fov = 50.0
    arr = sc.arrays()
    ctx.set_scene(arr)
    base = render(ctx, sc, 32, 32, 3)
    s0 = ctx.emitter_info()["sum_w"]
    # the emissive instance moves and grows: skh_update_accel
    inst = arr["instances"].copy()
    inst[e]["transform"] = (S.translate((0.7, -0.5, 0.2)) @ S.scale((1.5, 1.0, 1.0)))[:3].astype(np.float32).reshape(12)
    ctx.update_accel(inst)
    assert ctx.build_info()["refit"] == 2
    moved = render(ctx, sc, 32, 32, 3)
    arr1 = {**arr, "instances": inst}
    assert abs(ctx.emitter_info()["sum_w"] / s0 - 1.5) < 1e-5
    assert not np.array_equal(moved, base) and np.array_equal(moved, fresh_image(arr1, sc))
    # its vertices are edited: skh_set_geometry + skh_refit_accel
    v = arr["vertices"].copy()
    me = arr["meshes"][arr["instances"][e]["geom_id"]]
    sl = slice(int(me["vertex_offset"]), int(me["vertex_offset"]) + int(me["vertex_count"]))
    v["pos"][sl, 0] *= np.float32(0.5)
    arr2 = {**arr1, "vertices": v}
    ctx.set_geometry(arr2)
    ctx.refit_accel()
    edited = render(ctx, sc, 32, 32, 3)
    assert abs(ctx.emitter_info()["sum_w"] / s0 - 0.75) < 1e-5
    assert not np.array_equal(edited, moved) and np.array_equal(edited, fresh_image(arr2, sc))
    # the materials are replaced by a shorter list: the instance's material id now falls back to material 0, which emits another colour
    mats = arr["materials"][:1].copy()
    arr3 = {**arr2, "materials": mats, "emission": np.float32([[1.0, 2.0, 3.0]])}
    ctx.set_emission(None)
    ctx.set_materials(mats)
    ctx.set_emission(arr3["emission"])
    swapped = render(ctx, sc, 32, 32, 3)
    assert ctx.emitter_info()["triangles"] == 320 + 2  # the floor emits too now
    assert not np.array_equal(swapped, edited) and np.array_equal(swapped, fresh_image(arr3, sc))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: scheduling and hierarchy options
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bake", [4, 0])
def test_options_leave_an_emitter_lit_image_bit_identical(ctx, bake):
    """the options tests/test_gpu_env.py::test_options_leave_an_environment_lit_image_bit_identical runs -- speculation, sub-frame batches, tile sharding --,
    once on the baked world-space hierarchy and once with bake_world 0 (a top level; the table is in world space either way)"""
    sc = scenes.cornell_box()
    arr = sc.arrays()
    em = np.zeros((len(arr["materials"]), 3), np.float32)
    em[int(arr["instances"][0]["material_id"]) % len(em)] = (1.5, 1.0, 0.5)
    arr = {**arr, "emission": em}
    ctx.set_option("bake_world", bake)
    ctx.set_scene(arr)
    assert ctx.emitter_info()["triangles"] > 0
    w, h, spp = 64, 48, 12

    def frame(batch=None):
        ctx.resize(w, h)
        if batch is None:
            return render(ctx, sc, w, h, spp)
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
    # a new emission between two sub-frames of a speculated frame shows in the very next one
    import torch

    P = lambda i: S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=spp, max_depth=4)
    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    images = []
    for spec in (8, 0):
        ctx.set_option("speculate", spec)
        ctx.set_emission(em)
        ctx.resize(w, h)
        ctx.reset_stats()
        for i in range(5):
            ctx.render_subframe(P(i), img.data_ptr())
        ctx.set_emission(em * np.float32(4.0))
        ctx.render_subframe(P(5), img.data_ptr())
        images.append(ctx.read_accum()[..., :3].copy())
        if spec:
            assert ctx.stats()["speculated_discarded"] > 0
    assert np.array_equal(images[0], images[1])
    ctx.set_option("speculate", 8)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9: bad input
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_and_the_context_stays_usable(ctx):
    from strelka_amd import capi

    sc = scenes.cornell_box()
    arr = sc.arrays()
    ctx.set_scene(arr)
    nm = len(arr["materials"])
    with pytest.raises(capi.SkhError, match="no emitter"):
        ctx.emitter_probe("sample", np.zeros((1, 6), np.float32))
    good = np.zeros((nm, 3), np.float32)
    good[0] = (1.0, 2.0, 3.0)
    ctx.set_emission(good)
    info = ctx.emitter_info()
    a = render(ctx, sc, 32, 32, 2)
    for bad, what in ((np.where(np.arange(nm * 3).reshape(nm, 3) == 1, -1.0, good), "finite and >= 0"), (np.where(np.arange(nm * 3).reshape(nm, 3) == 2, np.nan, good), "finite and >= 0"),
                      (np.where(np.arange(nm * 3).reshape(nm, 3) == 0, np.inf, good), "finite and >= 0"), (np.ones((nm + 1, 3)), "materials")):
        with pytest.raises(capi.SkhError, match=what) as ei:
            ctx.set_emission(bad.astype(np.float32))
        assert "(3)" in str(ei.value)  # SKH_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ctx.set_emission(np.ones((nm, 4), np.float32))
    with pytest.raises(capi.SkhError):
        ctx.set_option("emit_nee", 2)
    assert ctx.emitter_info() == {**info, "ms_build": ctx.emitter_info()["ms_build"]}  # the previous emission is in place
    assert np.array_equal(render(ctx, sc, 32, 32, 2), a) and np.isfinite(a).all()
