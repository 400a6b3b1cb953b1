"""Inputs the hierarchy builders handle worst, and who must answer on each of them ("Every primitive is in the hierarchy").

A dropped primitive is silent: no comparison with an oracle that was given the same scene notices it unless a test ray happens to land on that primitive.  So
every scene here comes with a ROLL CALL: one short ray per primitive (three per triangle of box_twins, two per instance of the rows) that only that primitive can
answer, by construction, and the (instance, primitive), t, u, v a plain float64 intersection gives for it.  numpy only; of the product it reads the record layouts
(strelka_amd.scene) and nothing else.  tests/test_build_edges_cpu.py holds the generators, the reference and the checker's trace against each other on the CPU,
tests/test_gpu_build_edges.py holds the device's builders to the roll call.

The families (a Case = meshes + instances + curves, the roll-call rays, and per ray the expected instance and primitive):
  soup(n, seed)          one triangle in each of n cells of a unit lattice (cells in shuffled order: the primitive order is not the Morton order), centre jittered by
                         <= 0.1, circumradius 0.2 (edge 0.346 <= 0.4), random orientation: nothing of it leaves the ball of radius 0.3 about the cell's centre
  strip(n)               n / 2 unit quads in a row along x, two triangles each, shared vertices: coordinates are small integers, the ties exact in float32
  box_twins(n)           n triangles on the edge (0,0,0)-(1,1,1), third vertex on the circle of radius 0.6 about the diagonal's midpoint, in the plane across it (the
                         cube's hexagonal section has inradius 0.612): every box is [0,1]^3 bit for bit, the triangles share the diagonal and nothing else
  row_of_instances(n)    a 12-triangle cube of half-edge 0.25, n instances at spacing 1 along x (jitter > 0: a lattice twin with that much jitter per axis)
  long_strand(segments)  one straight uniform cubic B-spline strand along x, control points at spacing 1, radius 0.1
Decorations, Case -> Case: with_degenerates (zero-area triangles mixed into mesh 0: never reported), with_duplicates (exact repeats in mesh 0: the smaller
(instance, primitive) key answers), as_groups (every triangle of mesh 0 a mesh of its own under an identity instance), inside_soup (the case's mesh among a few soups).

The rays.  For a triangle the target is an interior point with every barycentric weight >= 0.2; the ray starts at target + h n (n the unit normal), runs along -n
with tmin 0 and tmax 2 h.  h comes from the construction: 0.15 in a soup (the ray stays within 0.25 of the cell's centre, every other triangle outside 0.7 of it),
0.25 on the strip (a planar strip: the ray meets the plane once, inside one triangle), 0.1 on a cube's top face (the faces next to it are 0.5 below and 0.5 aside),
and 0.1 of the gap between two sheets of the fan at the target on box_twins (8194 sheets: the gap is 1.8e-4 at weight 0.4 of the third vertex, h = 1.8e-5).
A strand's ray crosses the axis at right angles at the segment's mid-parameter from 4 radii away.

The reference (roll_call): the float32 vertices pushed through the float32 instance matrix in float64, Moeller-Trumbore in float64 on the float32 ray.  brute() tests
every ray against every triangle of the scene (n <= BRUTE_MAX triangles; chunked) and keeps a ray only if its own triangle is the one hit in the interval and no
other triangle comes within MARGIN_ULPS float32 ulps -- of the largest coordinate among the ray's origin and that triangle's vertices -- of being hit: its plane is
crossed that near the interval AND the crossing lies that near its inside (the distance to an edge: the weight times the altitude).  At most MAX_EXCLUDED of a
scene's rays may fail that, and every primitive keeps a ray: the CPU test asserts both for every scene the GPU test uses.

ploc_rounds restates the cluster selection of skh_bvh.h's k_ploc_nn / k_ploc_merge for one group under both tie rules and lbvh_ploc's switch between them; it documents why the GPU test's sizes were
chosen (docs/LOG.md "tied boxes") and is not a check of the device."""
import functools

import numpy as np

from strelka_amd import scene as S

BRUTE_MAX = 8200  # triangles up to which brute() is run
MARGIN_ULPS = 1e3
MAX_EXCLUDED = 0.02
ULP = 2.0 ** -23


class Case:
    """meshes: [(positions (V, 3) float32, triangles (T, 3))];  instances: [(type, geometry id, 3 x 4 matrix)] (None = identity);  strand: (points (P, 3), radius) or None;
    rays: S.RAY records;  inst, prim: per ray, who answers;  alt: per ray, other (instance, primitive) keys that coincide with it (with_duplicates);
    h: per ray, half its interval;  miss: rays that must hit nothing (with_degenerates)"""

    def __init__(self, meshes, instances, rays, inst, prim, h, strand=None, alt=None, miss=None, name=""):
        self.meshes, self.instances, self.strand, self.name = meshes, instances, strand, name
        self.rays, self.inst, self.prim, self.h = rays, np.asarray(inst, np.int64), np.asarray(prim, np.int64), np.asarray(h, np.float64)
        self.alt = alt if alt is not None else {}
        self.miss = miss if miss is not None else np.zeros(0, S.RAY)

    @property
    def triangles(self):
        """triangles handed in: every mesh's, once (what skh_build_info counts under bake_world 0 is per mesh, not per instance)"""
        return sum(len(t) for _, t in self.meshes)

    def arrays(self):
        """the flat arrays of Scene.arrays(): one default material, no lights, no textures"""
        nv = [len(p) for p, _ in self.meshes]
        verts = np.zeros(sum(nv), S.VERTEX)
        if nv:
            verts["pos"] = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p, _ in self.meshes])
        meshes = np.zeros(len(self.meshes), S.MESH)
        idx, io, vo = [], 0, 0
        for k, (p, t) in enumerate(self.meshes):
            meshes[k] = (io, 3 * len(t), vo, len(p))
            idx.append(np.asarray(t, np.uint32).reshape(-1))
            io, vo = io + 3 * len(t), vo + len(p)
        inst = np.zeros(len(self.instances), S.INSTANCE)
        ident = np.eye(4, dtype=np.float32)[:3].reshape(12)
        inst["transform"] = np.stack([ident if m is None else np.asarray(m, np.float32).reshape(12) for _, _, m in self.instances]) if len(inst) else 0
        inst["type"] = [t for t, _, _ in self.instances]
        inst["geom_id"] = [g for _, g, _ in self.instances]
        inst["light_id"] = S.NO_ID
        mats = np.zeros(1, S.MATERIAL)
        mats[0]["base_color"] = 0.8
        out = {"vertices": verts, "indices": np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0), np.uint32), "meshes": meshes,
               "curves": np.zeros(0, S.CURVE), "curve_points": np.zeros((0, 3), np.float32), "curve_radii": np.zeros(0, np.float32),
               "curve_vertex_counts": np.zeros(0, np.uint32), "instances": inst, "lights": np.zeros(0, S.LIGHT), "materials": mats, "textures": []}
        if self.strand is not None:
            pts, radius = self.strand
            out["curves"] = np.zeros(1, S.CURVE)
            out["curves"][0] = (0, 1, 0, len(pts), 0, len(pts))
            out["curve_points"] = np.ascontiguousarray(pts, np.float32)
            out["curve_radii"] = np.full(len(pts), radius, np.float32)
            out["curve_vertex_counts"] = np.array([len(pts)], np.uint32)
        return out


def _rays(origin, direction, tmax):
    r = np.zeros(len(origin), S.RAY)
    r["origin"], r["dir"], r["tmax"] = origin, direction, tmax
    return r


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _roll_rays(P, weights, h):
    """P (T, 3, 3) float32 world-space vertices, weights (K, 3), h (T,) or scalar -> rays (T * K, triangle-major), the triangle of each ray, h of each ray"""
    P = np.asarray(P, np.float64)
    w = np.asarray(weights, np.float64)
    n = _unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    target = np.einsum("kv,tvc->tkc", w, P)
    hh = np.broadcast_to(np.asarray(h, np.float64).reshape(-1, 1), target.shape[:2])
    o = target + hh[..., None] * n[:, None, :]
    d = np.broadcast_to(-n[:, None, :], o.shape)
    tri = np.repeat(np.arange(len(P)), len(w))
    return _rays(o.reshape(-1, 3), d.reshape(-1, 3), 2.0 * hh.reshape(-1)), tri, hh.reshape(-1).copy()


CENTROID = [(1 / 3, 1 / 3, 1 / 3)]
MESH, CURVE = S.INSTANCE_MESH, S.INSTANCE_CURVE


def _soup_triangles(n, seed, origin=(0.0, 0.0, 0.0)):
    rs = np.random.RandomState(seed)
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    while side ** 3 < n:
        side += 1
    cells = rs.permutation(side ** 3)[:n]
    c = np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1) + 0.5 + rs.uniform(-0.1, 0.1, (n, 3)) + np.asarray(origin)
    a = _unit(rs.normal(size=(n, 3)))
    b = _unit(np.cross(a, rs.normal(size=(n, 3))))
    ang = rs.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])[None, :]
    P = c[:, None, :] + 0.2 * (np.cos(ang)[..., None] * a[:, None, :] + np.sin(ang)[..., None] * b[:, None, :])
    return P.astype(np.float32)


def soup(n, seed=1):
    P = _soup_triangles(n, seed)
    rays, tri, h = _roll_rays(P, CENTROID, 0.15)
    return Case([(P.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))], [(MESH, 0, None)], rays, np.zeros(len(tri)), tri, h, name="soup(%d)" % n)


def strip(n, jitter=0.0, wave=0.0, seed=5):
    """jitter > 0: the twin with every vertex moved by up to that much in x and y (docs/LOG.md's build-time ratio; h and the construction hold up to 0.1);
    wave > 0: the strip after a smooth displacement of that amplitude that breaks every tie (the refit's edit; a height field of slope < 0.4 wave: up to 0.1)"""
    assert n % 2 == 0 and n >= 2
    q = n // 2
    x = np.arange(q + 1, dtype=np.float64)
    pos = np.concatenate([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1, 0 * x], 1)])
    if jitter:
        pos[:, :2] += np.random.RandomState(seed).uniform(-jitter, jitter, (len(pos), 2))
    if wave:
        pos[:, 2] += wave * np.sin(0.37 * pos[:, 0] + 0.9 * pos[:, 1])
        pos[:, 1] += 0.5 * wave * np.cos(0.11 * pos[:, 0])
    pos = pos.astype(np.float32)
    k = np.arange(q)
    tris = np.empty((n, 3), np.int64)
    tris[0::2] = np.stack([k, k + 1, q + 1 + k + 1], 1)
    tris[1::2] = np.stack([k, q + 1 + k + 1, q + 1 + k], 1)
    rays, tri, h = _roll_rays(pos[tris], CENTROID, 0.25)
    return Case([(pos, tris)], [(MESH, 0, None)], rays, np.zeros(len(tri)), tri, h, name="strip(%d%s%s)" % (n, ", jittered" if jitter else "", ", waved" if wave else ""))


TWIN_WEIGHTS = [(0.2, 0.2, 0.6), (0.4, 0.2, 0.4), (0.2, 0.4, 0.4)]  # (weights of the diagonal's two ends, of the third vertex)
TWIN_RADIUS = 0.6


def box_twins(n):
    phi = 2 * np.pi * np.arange(n) / n
    e1, e2 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    third = 0.5 + TWIN_RADIUS * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    P = np.zeros((n, 3, 3))
    P[:, 1] = 1.0
    P[:, 2] = third
    P = P.astype(np.float32)
    w = np.asarray(TWIN_WEIGHTS)
    # the gap between two sheets at a target: its distance from the diagonal (weight x circle radius) times the fan's angular step
    gap = w[:, 2] * TWIN_RADIUS * 2 * np.pi / max(n, 4)
    rays, tri, h = _roll_rays(P, w, 0.01)
    hh = np.tile(0.1 * gap, n)
    nrm = -np.asarray(rays["dir"], np.float64)
    target = np.asarray(rays["origin"], np.float64) - 0.01 * nrm
    rays = _rays(target + hh[:, None] * nrm, -nrm, 2.0 * hh)
    return Case([(P.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))], [(MESH, 0, None)], rays, np.zeros(len(tri)), tri, hh, name="box_twins(%d)" % n)


CUBE_HALF = 0.25


def _cube():
    s = CUBE_HALF
    pos = np.array([(x, y, z) for z in (-s, s) for y in (-s, s) for x in (-s, s)], np.float32)
    quads = [(4, 5, 7, 6), (0, 2, 3, 1), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # +z first: triangles 0 and 1 are the top face
    tris = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)
    return pos, tris


def row_positions(n, spacing=1.0, jitter=0.0, seed=3):
    if jitter == 0.0:
        return np.stack([np.arange(n) * spacing, np.zeros(n), np.zeros(n)], 1)
    rs = np.random.RandomState(seed)
    side = 1
    while side ** 3 < n:
        side += 1
    cells = rs.permutation(side ** 3)[:n]
    return (np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1) + rs.uniform(-jitter, jitter, (n, 3))) * spacing


def row_of_instances(n, spacing=1.0, jitter=0.0):
    """n instances of one cube; the roll call: both triangles of every instance's top face.  jitter > 0: the lattice twin (cube 0.25 + jitter <= 0.2 stays in its cell)"""
    pos, tris = _cube()
    c = row_positions(n, spacing, jitter)
    M = np.tile(np.eye(4)[:3][None], (n, 1, 1))
    M[:, :, 3] = c
    M = M.astype(np.float32)
    top = np.asarray(pos[tris[:2]], np.float64)  # (2, 3, 3)
    W = top[None] + np.asarray(M[:, :, 3], np.float64)[:, None, None, :]  # (n, 2, 3, 3): a translation by the float32 column, in float64
    rays, tri, h = _roll_rays(W.reshape(-1, 3, 3), CENTROID, 0.1)
    return Case([(pos, tris)], [(MESH, 0, m) for m in M], rays, tri // 2, tri % 2, h, name="row_of_instances(%d%s)" % (n, ", jittered" if jitter else ""))


STRAND_RADIUS = 0.1


def long_strand(segments):
    """control point k at x = k: segment i runs over x in [i + 1, i + 2], linearly in u; its ray comes down the z axis onto x = i + 1.5 from 4 radii off the axis"""
    pts = np.stack([np.arange(segments + 3, dtype=np.float64), np.zeros(segments + 3), np.zeros(segments + 3)], 1).astype(np.float32)
    x = np.arange(segments) + 1.5
    o = np.stack([x, 0 * x, 0 * x + 4 * STRAND_RADIUS], 1)
    rays = _rays(o, np.broadcast_to([0.0, 0.0, -1.0], o.shape), 8 * STRAND_RADIUS)
    return Case([], [(CURVE, 0, None)], rays, np.zeros(segments), np.arange(segments), np.full(segments, 4 * STRAND_RADIUS), strand=(pts, STRAND_RADIUS),
                name="long_strand(%d)" % segments)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# decorations
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mesh0_rays(case):
    """the rays whose expected triangle lies in mesh 0 (under instance 0, the only user of mesh 0 in the cases the decorations take)"""
    assert case.instances[0][1] == 0 and sum(1 for t, g, _ in case.instances if t == MESH and g == 0) == 1
    return case.inst == 0


def _interleave(rs, n_old, n_new):
    """new triangles mixed into the old order at random places, the old ones keeping their relative order -> (slot of each old, slot of each new)"""
    slots = np.sort(rs.permutation(n_old + n_new)[:n_new])
    is_new = np.zeros(n_old + n_new, bool)
    is_new[slots] = True
    return np.nonzero(~is_new)[0], slots


def with_degenerates(case, k, seed=7):
    """k zero-area triangles in mesh 0, half with two equal vertices and half with three collinear ones, each halfway down the roll-call ray of a real triangle (inside
    the interval that holds nothing else): the ray through it must still report the real triangle, and `miss` -- the same line, ending a quarter of the interval
    before the real triangle -- must report nothing.  (The degenerate's first vertex lies ON both rays.)"""
    rs = np.random.RandomState(seed)
    pos, tris = case.meshes[0]
    mine = np.nonzero(_mesh0_rays(case))[0]
    pick = mine[rs.permutation(len(mine))[:k]] if k <= len(mine) else mine[rs.randint(0, len(mine), k)]
    o, d, h = np.asarray(case.rays["origin"], np.float64)[pick], np.asarray(case.rays["dir"], np.float64)[pick], case.h[pick]
    q = o + 0.5 * h[:, None] * d  # (the instance of mesh 0 is the identity: world space is object space)
    assert case.instances[0][2] is None
    e = np.zeros_like(q)
    e[:, 0] = 0.25 * h  # (along x: three points that differ in one coordinate are collinear in float32 whatever that coordinate rounds to)
    two_equal = (np.arange(k) % 2) == 0
    V = np.stack([q, np.where(two_equal[:, None], q, q - e), q + e], 1).astype(np.float32)
    old_slot, new_slot = _interleave(rs, len(tris), k)
    nt = np.empty((len(tris) + k, 3), np.int64)
    nt[old_slot] = tris
    nt[new_slot] = len(pos) + np.arange(3 * k).reshape(k, 3)
    prim = case.prim.copy()
    prim[mine] = old_slot[case.prim[mine]]
    q32 = np.asarray(V[:, 0], np.float64)
    miss = _rays(q32 - 0.25 * h[:, None] * d, d, 0.5 * h)
    alt = {r: [(i, int(old_slot[p]) if i == 0 else p) for i, p in keys] for r, keys in case.alt.items()}
    return Case([(np.concatenate([pos, V.reshape(-1, 3)]), nt)] + case.meshes[1:], case.instances, case.rays, case.inst, prim, case.h, case.strand, alt,
                np.concatenate([case.miss, miss]), case.name + " + %d degenerate" % k)


def with_duplicates(case, k, seed=9):
    """k triangles of mesh 0 repeated exactly (the same three vertex indices) at random places of its index buffer: their rays meet two coincident triangles, and
    the smaller primitive index must answer (equal t -> the smaller (instance, primitive) key)"""
    rs = np.random.RandomState(seed)
    pos, tris = case.meshes[0]
    mine = np.nonzero(_mesh0_rays(case))[0]
    called = np.unique(case.prim[mine])  # (the triangles with a ray: not the degenerate ones)
    src = called[rs.permutation(len(called))[:k]] if k <= len(called) else called[rs.randint(0, len(called), k)]
    old_slot, new_slot = _interleave(rs, len(tris), len(src))
    nt = np.empty((len(tris) + len(src), 3), np.int64)
    nt[old_slot] = tris
    nt[new_slot] = tris[src]
    copies = {}
    for s, slot in zip(src, new_slot):
        copies.setdefault(int(s), []).append(int(slot))
    prim = case.prim.copy()
    alt = {}
    for r in mine:
        p = int(case.prim[r])
        keys = [int(old_slot[p])] + copies.get(p, [])
        prim[r] = min(keys)
        if len(keys) > 1:
            alt[int(r)] = [(0, s) for s in keys]
    return Case([(pos, nt)] + case.meshes[1:], case.instances, case.rays, case.inst, prim, case.h, case.strand, alt, case.miss, case.name + " + %d repeated" % k)


def as_groups(case):
    """every triangle of mesh 0 a mesh of its own, instanced with the identity: n groups of one triangle; triangle j answers as (instance j, primitive 0)"""
    assert len(case.meshes) == 1 and len(case.instances) == 1 and case.instances[0][2] is None
    pos, tris = case.meshes[0]
    meshes = [(pos[t], np.array([[0, 1, 2]])) for t in tris]
    alt = {r: [(p, 0) for _, p in keys] for r, keys in case.alt.items()}
    return Case(meshes, [(MESH, j, None) for j in range(len(tris))], case.rays, case.prim, np.zeros_like(case.prim), case.h, None, alt, case.miss,
                case.name + " as groups")


def inside_soup(case, n_soups=3, n=300, seed=21):
    """the case's mesh (instance 0) among a few soup meshes placed beside it: in key order the group's neighbours are other groups.  The soups sit beyond x, y, z <
    -1 (the cases live in x, y, z >= -0.5); their triangles join the roll call."""
    meshes, instances = list(case.meshes), list(case.instances)
    rays, inst, prim, h = [case.rays], [case.inst], [case.prim], [case.h]
    for k in range(n_soups):
        side = int(np.ceil(n ** (1.0 / 3.0)))
        P = _soup_triangles(n, seed + k, origin=(-1.5 - side, -1.5 - side - k * (side + 1), -1.5 - side))
        r, tri, hh = _roll_rays(P, CENTROID, 0.15)
        meshes.append((P.reshape(-1, 3), np.arange(3 * n).reshape(n, 3)))
        instances.append((MESH, len(meshes) - 1, None))
        rays.append(r), inst.append(np.full(len(tri), len(instances) - 1)), prim.append(tri), h.append(hh)
    return Case(meshes, instances, np.concatenate(rays), np.concatenate(inst), np.concatenate(prim), np.concatenate(h), case.strand, case.alt, case.miss,
                case.name + " among %d soups" % n_soups)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def world_triangles(arr):
    """(instance, primitive, world-space vertices (T, 3, 3) float64) of every triangle of every mesh instance: float32 data, float64 arithmetic"""
    inst, prim, W = [], [], []
    V = np.asarray(arr["vertices"]["pos"], np.float64)
    order = np.argsort(arr["instances"]["geom_id"], kind="stable")
    for i in order:  # (grouped by mesh only to gather each mesh's vertices once; the table is sorted back below)
        rec = arr["instances"][i]
        if int(rec["type"]) != MESH:
            continue
        me = arr["meshes"][int(rec["geom_id"])]
        idx = arr["indices"][int(me["index_offset"]):int(me["index_offset"]) + int(me["index_count"])].astype(np.int64).reshape(-1, 3) + int(me["vertex_offset"])
        M = np.asarray(rec["transform"], np.float64).reshape(3, 4)
        W.append(V[idx] @ M[:, :3].T + M[:, 3])
        inst.append(np.full(len(idx), i)), prim.append(np.arange(len(idx)))
    if not W:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3, 3))
    inst, prim, W = np.concatenate(inst), np.concatenate(prim), np.concatenate(W)
    k = np.lexsort((prim, inst))
    return inst[k], prim[k], W[k]


def _moeller(o, d, W):
    """row-wise: ray r against triangle W[r] -> t, u (second vertex), v (third vertex), det; nan where the ray is parallel to the plane or the triangle has no area"""
    e1, e2 = W[:, 1] - W[:, 0], W[:, 2] - W[:, 0]
    n = np.cross(e1, e2)
    s = o - W[:, 0]
    det = -(d * n).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        q = np.cross(s, d)
        return (s * n).sum(1) * inv, (q * e2).sum(1) * inv, -(q * e1).sum(1) * inv, det


def roll_call(case, arr=None):
    """the reference's answer per ray: inst, prim (the expected key: the smallest of coincident ones), t, u, v, and L = the largest coordinate in play, alt = the
    triangle's smallest altitude (the scale of hitref's bars).  Curves: tests/curveref.py's entry into the strand."""
    arr = arr if arr is not None else case.arrays()
    o, d = np.asarray(case.rays["origin"], np.float64), np.asarray(case.rays["dir"], np.float64)
    if case.strand is not None:
        from tests import curveref

        r = curveref.trace(arr, case.rays)
        return {"inst": np.where(r["hit"], r["inst"], -1), "prim": np.where(r["hit"], r["seg"], -1), "t": r["t"], "u": r["u_foot"], "v": np.zeros(len(o)), "curve": r}
    inst, prim, W = world_triangles(arr)
    first = np.concatenate([[0], np.cumsum(np.bincount(inst, minlength=len(arr["instances"])))[:-1]])
    row = first[case.inst] + case.prim
    assert np.array_equal(inst[row], case.inst) and np.array_equal(prim[row], case.prim)
    t, u, v, _ = _moeller(o, d, W[row])
    Wr = W[row]
    a, b, c = Wr[:, 1] - Wr[:, 0], Wr[:, 2] - Wr[:, 0], Wr[:, 2] - Wr[:, 1]
    longest = np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), np.linalg.norm(c, axis=1))
    return {"inst": case.inst, "prim": case.prim, "t": t, "u": u, "v": v, "row": row, "L": np.maximum(np.abs(Wr).max(axis=(1, 2)), np.abs(o).max(axis=1)),
            "alt": np.linalg.norm(np.cross(a, b), axis=1) / longest}


def brute(case, arr=None, chunk=512):
    """-> keep (N,) bool: the ray's own triangle (and its exact repeats) is the only one of the whole scene hit in [0, 2 h], with every weight >= 0.2 - 1e-6, and no
    other triangle comes within MARGIN_ULPS ulps of it (module docstring).  Every ray against every triangle, float64."""
    arr = arr if arr is not None else case.arrays()
    inst, prim, W = world_triangles(arr)
    ref = roll_call(case, arr)
    o, d = np.asarray(case.rays["origin"], np.float64), np.asarray(case.rays["dir"], np.float64)
    tmax = np.asarray(case.rays["tmax"], np.float64)
    own_ok = (ref["t"] > 0) & (ref["t"] < tmax) & (np.minimum(np.minimum(ref["u"], ref["v"]), 1 - ref["u"] - ref["v"]) >= 0.2 - 1e-6)
    first = np.concatenate([[0], np.cumsum(np.bincount(inst, minlength=len(arr["instances"])))[:-1]])
    e1, e2 = W[:, 1] - W[:, 0], W[:, 2] - W[:, 0]
    n = np.cross(e1, e2)
    area2 = np.linalg.norm(n, axis=1)
    nW0 = (n * W[:, 0]).sum(1)
    Lt = np.abs(W).max(axis=(1, 2))
    keep = own_ok.copy()
    for s in range(0, len(o), chunk):
        oo, dd = o[s:s + chunk], d[s:s + chunk]
        det = -(dd @ n.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (oo @ n.T - nW0[None, :]) / det  # (unit directions: t is a length)
        delta = MARGIN_ULPS * ULP * np.maximum(np.abs(oo).max(axis=1)[:, None], Lt[None, :])
        near = (det != 0) & (area2[None, :] > 0) & (t >= -delta) & (t <= tmax[s:s + chunk, None] + delta)
        near[np.arange(len(oo)), ref["row"][s:s + chunk]] = False
        for r, keys in case.alt.items():
            if s <= r < s + chunk:
                for i, p in keys:
                    near[r - s, first[i] + p] = False
        rr, tt = np.nonzero(near)
        if not len(rr):
            continue
        _, u, v, _ = _moeller(oo[rr], dd[rr], W[tt])
        mb = np.minimum(np.minimum(u, v), 1 - u - v)
        a, b, c = e1[tt], e2[tt], W[tt, 2] - W[tt, 1]
        altitude = area2[tt] / np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), np.linalg.norm(c, axis=1))
        bad = mb * altitude >= -delta[rr, tt]
        keep[s + rr[bad]] = False
    return keep


def check_cover(case, keep):
    """the two conditions on what brute() leaves out: at most MAX_EXCLUDED of the rays, and every primitive of the roll call keeps a ray -> (share left out, primitives without a ray)"""
    keys = case.inst * (1 << 32) + case.prim
    return 1.0 - keep.mean(), len(np.setdiff1d(np.unique(keys), np.unique(keys[keep])))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cluster selection of the PLOC builder, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------
def morton_order(lo, hi, bits=10):
    """the order the builder clusters one group in: k_morton's code of the box centres inside the group's bounds (float32 arithmetic), a stable sort"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    c = np.float32(0.5) * (lo + hi)
    b0, b1 = lo.min(axis=0), hi.max(axis=0)
    e = b1 - b0
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(e > 0, (c - b0) / e, np.float32(0)).astype(np.float32)
    cells = np.float32(1 << bits)
    q = np.minimum(np.maximum(nrm * cells, np.float32(0)), cells - np.float32(1)).astype(np.uint64)
    code = np.zeros(len(lo), np.uint64)
    for bit in range(bits):
        for axis, sh in ((0, 2), (1, 1), (2, 0)):
            code |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + sh)
    return np.argsort(code, kind="stable")


def _choose(lo, hi, idx, radius, rule):
    """the partner each cluster of `idx` names (k_ploc_nn): the smallest float32 half-area ex ey + ey ez + ez ex of the merged box among the `radius` neighbours on
    either side; ties -- rule "lowest": the first of the scan from -radius to +radius; rule "paired": the nearer, then the side floor(i / k) names"""
    m = len(lo)
    best = np.full(len(idx), np.inf, np.float32)
    who = np.full(len(idx), -1, np.int64)

    def offer(dd):
        j = idx + dd
        ok = (j >= 0) & (j < m)
        jj = np.where(ok, j, 0)
        ext = np.maximum(hi[idx], hi[jj]) - np.minimum(lo[idx], lo[jj])
        cost = np.where(ok, ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0], np.float32(np.inf))
        better = cost < best
        best[better], who[better] = cost[better], j[better]

    if rule == "lowest":
        for dd in range(-radius, radius + 1):
            if dd:
                offer(dd)
    else:
        assert rule == "paired"
        for k in range(1, radius + 1):
            first = np.where((idx // k) & 1, -k, k)
            offer(first)
            offer(-first)
    return who


def ploc_rounds(lo, hi, radius, rule, cap=4096, incremental=True):
    """rounds of k_ploc_nn + k_ploc_merge it takes to bring the clusters lo, hi (float32 boxes of ONE group, already in cluster order) down to one, and how many
    are left when `cap` rounds are used up -> (rounds, clusters left).  rule: "lowest" (the old one throughout), "paired" (the new one throughout), "adaptive" (what
    lbvh_ploc does: "lowest" until two rounds in a row each do less than a sixteenth of the merges still to do, "paired" from then on).  incremental: under "lowest" a cluster names a
    new partner only when its window changed (the result is the same -- tests/test_build_edges_cpu.py compares -- and a chain of 4096 one-merge rounds over 32 k
    clusters takes seconds, not minutes)."""
    lo, hi = np.array(lo, np.float32), np.array(hi, np.float32)
    m = len(lo)
    now = "paired" if rule == "paired" else "lowest"
    nn = _choose(lo, hi, np.arange(m), radius, now)
    rounds = slow = 0
    while m > 1 and rounds < cap:
        i = np.arange(m)
        pair = (nn >= 0) & (nn[np.maximum(nn, 0)] == i)
        lower, upper = pair & (i < nn), pair & (i > nn)
        if not lower.any():
            break
        rounds += 1
        j = nn[lower]
        lo[lower], hi[lower] = np.minimum(lo[lower], lo[j]), np.maximum(hi[lower], hi[j])
        keepm = ~upper
        pos = np.cumsum(keepm) - 1
        # a cluster's choice stands while its window holds the same clusters at the same offsets: none merged, none removed within radius + 1 of it
        touched = np.zeros(m - int(upper.sum()), bool)
        touched[pos[lower]] = True
        gone = np.nonzero(upper)[0]
        touched[np.clip(pos[gone], 0, len(touched) - 1)] = True
        touched[np.clip(pos[gone] + 1, 0, len(touched) - 1)] = True
        off = nn - i
        slow = slow + 1 if int(upper.sum()) * 16 < m - 1 else 0  # (m - 1: the merges still to do in one group)
        if rule == "adaptive" and slow >= 2:
            now = "paired"
        lo, hi, off = lo[keepm], hi[keepm], off[keepm]
        m = len(lo)
        if incremental and now == "lowest":  # ("paired" reads the cluster's own index, which every removal to its left shifts; it needs few rounds anyway)
            csum = np.concatenate([[0], np.cumsum(touched)])
            a, b = np.clip(np.arange(m) - radius - 1, 0, m), np.clip(np.arange(m) + radius + 2, 0, m)
            dirty = np.nonzero(csum[b] > csum[a])[0]
            nn = np.arange(m) + off
            nn[dirty] = _choose(lo, hi, dirty, radius, now)
        else:
            nn = _choose(lo, hi, np.arange(m), radius, now)
    return rounds, m


def boxes_of(case):
    """float32 boxes of the case's mesh-0 triangles (object space), or of its instances' cubes"""
    pos, tris = case.meshes[0]
    if len(case.instances) > 1:
        c = np.stack([np.asarray(m, np.float32)[:, 3] for _, _, m in case.instances])
        return (c - np.float32(CUBE_HALF)).astype(np.float32), (c + np.float32(CUBE_HALF)).astype(np.float32)
    P = np.asarray(pos, np.float32)[tris]
    return P.min(axis=1), P.max(axis=1)


@functools.lru_cache(maxsize=None)
def cached(name, *args):
    """a family by name with its arrays, reference and brute-force verdict, made once per process: (case, arrays, reference, keep or None)"""
    case = FAMILIES[name](*args)
    arr = case.arrays()
    ref = roll_call(case, arr)
    n_tris = sum(len(case.meshes[g][1]) for t, g, _ in case.instances if t == MESH)
    keep = brute(case, arr) if case.strand is None and n_tris <= BRUTE_MAX else None
    return case, arr, ref, keep


FAMILIES = {
    "soup": soup,
    "soup_groups": lambda n, seed=1: as_groups(soup(n, seed)),
    "soup_decorated": lambda n, k: with_duplicates(with_degenerates(soup(n), k), k),
    "soup_groups_decorated": lambda n, k: as_groups(with_duplicates(with_degenerates(soup(n), k), k)),
    "strip": strip,
    "strip_decorated": lambda n, k: with_duplicates(with_degenerates(strip(n), k), k),
    "strip_in_soup": lambda n: inside_soup(strip(n)),
    "box_twins": box_twins,
    "box_twins_in_soup": lambda n: inside_soup(box_twins(n)),
    "row": row_of_instances,
    "row_jittered": lambda n: row_of_instances(n, jitter=0.2),
    "long_strand": long_strand,
    "strip_waved": lambda n: strip(n, wave=0.05),
    "strip_jittered": lambda n: strip(n, jitter=0.1),
    "row_spaced": lambda n: row_of_instances(n, spacing=1.5),
}

# ---------------------------------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_build_edges.py builds (tests/test_build_edges_cpu.py holds the reference to its two conditions on every one of them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
# counts on a kernel's tail: one-primitive trees, the 64-lane wave, SKH_PLOC_BLOCK / SKH_LEAF_CHUNK 256, the 4096-key radix-sort and scan blocks, tlas_build 2's 8192
TAIL_COUNTS = [1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193]
TOP_COUNTS = [1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 16386]
DECORATED = [(225, 16), (4065, 16)]  # n real + 16 degenerate + 16 repeated triangles: 257 and 4097 handed in
TAIL_SCENES = [("soup", n) for n in TAIL_COUNTS] + [("soup_decorated", n, k) for n, k in DECORATED]
GROUP_SCENES = [("soup_groups", n) for n in TAIL_COUNTS if n <= 4097] + [("soup_groups_decorated", n, k) for n, k in DECORATED]
TOP_SCENES = [(f, n) for n in TOP_COUNTS for f in ("row", "row_jittered")]
TIED_SCENES = [("strip", 32770), ("box_twins", 8194), ("box_twins", 4097), ("strip_in_soup", 32770), ("box_twins_in_soup", 8194), ("box_twins_in_soup", 4097)]
STRAND_SCENES = [("long_strand", 4099)]
REFIT_SCENES = [("strip_waved", 32770), ("row", 8193), ("row_spaced", 8193)]
GPU_SCENES = TAIL_SCENES + GROUP_SCENES + TOP_SCENES + TIED_SCENES + STRAND_SCENES + REFIT_SCENES
