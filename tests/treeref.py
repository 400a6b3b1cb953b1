"""Scenes on which a hit record could depend on the tree, and a float64 reference that says which rays are decided ("Determinism rules";
docs/LOG.md "A hit record that depended on the tree").

The contract: closest hit = the smallest COMPUTED t, ties to the smaller (instance, primitive) key, whatever hierarchy is walked.  A node test that culls against the
best t so far may only skip a box none of whose triangles can compute a smaller t.  The intersector's t is (U Az + V Bz + W Cz) / (U + V + W) with the rounded edge
functions U, V, W in numerator and denominator alike: a weighted mean of the vertices' parametric depths along the ray's dominant axis with non-negative weights --
inside the triangle's slab on THAT axis whatever the weights' errors, and anywhere inside it on the other two once the weights are ill-conditioned (a sliver seen
along its plane: |det| << S).  The scenes here are the ones where that happens or where boxes are flat: metres-long two-triangle quads, coplanar overlapping panels,
50 : 1 ... 500 : 1 slats beside a wall, and the 1600 : 1 rod of the architectural kitchen whose record 865 showed it (mechanism_scene).

numpy only; of the product it reads the record layouts (strelka_amd.scene) through tests/buildref.py's Case and tests/hitref.py's triangle table.
tests/test_tree_independence_cpu.py holds the scenes, this reference and the checker against each other; tests/test_gpu_tree_independence.py holds the device's trees.

Geometry is exact: under a transform (flat_room's cabinets: translations by multiples of 1/4, scales 1 or 2) coordinates are multiples of 2^-10; everything else -- the panels
displaced by one ulp, the rods' rings -- is float32 as it comes under the identity.  Either way the float32 world-space vertex a baked build computes IS the float64 one (asserted in
world_triangles).

The bars (reference()).  u = 2^-24.  With the ray's shear (Sx, Sy, Sz) and A = p0 - o, ...:
  a sheared coordinate Ax = A.x - Sx A.z carries: the difference p - o (1 rounding), Sx = d.x (1 / d.z) (2), the product (1), the difference (1): <= 5 u X with
    X = max over the vertices of |A.x| + |Sx A.z| (Y likewise);
  an edge function U = Cx By - Cy Bx: two products and a difference, <= 3 u (|Cx By| + |Cy Bx|), and the coordinates' own errors,
    <= 5 u (X (|By| + |Cy|) + Y (|Bx| + |Cx|)); summed over U, V, W:  E = 3 u S + 10 u (X SY + Y SX),  SX = |Ax| + |Bx| + |Cx|, S = SX SY (the intersector's S);
  a weight U / det then moves by <= 2 E / |det| (its own error and the denominator's) + 2 u (reciprocal, product):   b_bar = (2 E / |det| + 2 u) / (1 - E / |det|);
  t is the weights' mean of Az, Bz, Cz: the weights' errors move it by <= (E / |det|) max |z_i - t| -- THE FAR-VERTEX TERM: the distance to the farthest vertex times the
    weights' conditioning --, each z_i = Sz (p.z - o.z) carries 3 roundings on |z_i| and the difference's u (|p.z| + |o.z|) |Sz|, the sum T three products and two sums,
    then the reciprocal and the product: 3 + 5 + 2 = 10 u max |z_i|;  on top hitref's C_ISECT u L for the coordinates' chain (L = the largest magnitude among the origin
    and the vertices, times |Sz| sqrt(3) to turn a displacement into t):
    t_bar = ((E / |det|) max |z_i - t| + 10 u max |z_i| + u (|p.z| + |o.z|)max |Sz| + C_ISECT u L |Sz| sqrt(3)) / (1 - E / |det|).
  Pairs with E / |det| > 1/4 have no bar (first order no longer holds): they are possible hits anywhere in their slab, never decided ones.
A ray is DECIDED when a triangle is hit for certain (U, V, W further than E from 0 on one side, t > 2 t_bar + the intersector's own rejection threshold 2^-20 S max |z| / |det|) and every
other triangle that may be hit (no weight further than E on the wrong side, t > -t_bar, and not |t| + t_bar < that threshold: an origin ON it) lies further than the sum of the two t bars behind it; or when no triangle may be hit at all."""
import functools
import os

import numpy as np

from strelka_amd import scene as S
from tests import buildref as B
from tests import hitref

U = hitref.U
MESH = S.INSTANCE_MESH
MAX_UNDECIDED = 0.02
MIN_HIT = 0.40
Q = 1024.0  # coordinates are multiples of 1 / Q


def _q(x):
    return np.round(np.asarray(x, np.float64) * Q) / Q


class Builder:
    """one mesh: vertices and triangles; quads are split along a chosen diagonal"""

    def __init__(self):
        self.v, self.t = [], []

    def quad(self, p, eu, ev, flip=False):
        p, eu, ev = np.asarray(p, np.float64), np.asarray(eu, np.float64), np.asarray(ev, np.float64)
        k = len(self.v)
        self.v += [p, p + eu, p + eu + ev, p + ev]
        self.t += [(k, k + 1, k + 3), (k + 1, k + 2, k + 3)] if flip else [(k, k + 1, k + 2), (k, k + 2, k + 3)]

    def box(self, lo, hi, flip=0):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        e = np.diag(hi - lo)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            self.quad(lo, e[b], e[c], bool((flip >> a) & 1))
            self.quad(lo + e[a], e[c], e[b], bool((flip >> (a + 3)) & 1))

    def cylinder(self, a, b, radius, segments, phase=0.0):
        """`segments` facets around, one along: two slivers per facet"""
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        ax = (b - a) / np.linalg.norm(b - a)
        e1 = np.cross(ax, [0.0, 0.0, 1.0] if abs(ax[2]) < 0.9 else [1.0, 0.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(ax, e1)
        ang = phase + 2 * np.pi * np.arange(segments) / segments
        ring = radius * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
        k = len(self.v)
        self.v += list(a + ring) + list(b + ring)  # (float32 as they come: a rod's instance has the identity transform)
        for i in range(segments):
            j = (i + 1) % segments
            self.t += [(k + i, k + j, k + segments + j), (k + i, k + segments + j, k + segments + i)] if i % 2 else [(k + i, k + j, k + segments + i), (k + j, k + segments + j, k + segments + i)]

    def mesh(self):
        return np.asarray(self.v, np.float32).reshape(-1, 3), np.asarray(self.t, np.int64).reshape(-1, 3)


def _translate(x, y, z, sx=1.0):
    return np.array([[sx, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], np.float32)


class Scene:
    """meshes [(positions float32, triangles)], instances [(type, mesh, 3 x 4 float32 matrix or None)], and what the ray generators need"""

    def __init__(self, name, meshes, instances, seed, rods=(), shares=None, avoid=(), n_rays=12000):
        self.name, self.meshes, self.instances, self.seed, self.rods = name, meshes, instances, seed, list(rods)
        self.shares, self.n_rays = shares or {}, n_rays
        self.avoid = np.asarray(avoid, np.int64)  # world triangles the general ray families do not aim at
        self._case = B.Case(meshes, instances, np.zeros(0, S.RAY), np.zeros(0), np.zeros(0), np.zeros(0), name=name)

    def arrays(self):
        return self._case.arrays()

    @property
    def triangles(self):
        return sum(len(self.meshes[g][1]) for _, g, _ in self.instances)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def flat_room():
    """a room of axis-aligned two-triangle quads 2 ... 8 long, on the coordinate planes (floor z = 0, walls x = 0 and y = 0) and off them, partitions and a table top
    inside it, and 19 cabinets (one mesh, translated; every fourth stretched to twice its width): an outer box, an inner box 1/64 inside it, three shelves 1/64 thick --
    every face a two-triangle quad, the diagonals alternating"""
    room = Builder()
    room.quad((0, 0, 0), (8, 0, 0), (0, 6, 0))
    room.quad((0, 0, 2.75), (0, 6, 0), (8, 0, 0), True)
    room.quad((0, 0, 0), (0, 6, 0), (0, 0, 2.75))
    room.quad((8, 0, 0), (0, 0, 2.75), (0, 6, 0), True)
    room.quad((0, 0, 0), (0, 0, 2.75), (8, 0, 0))
    room.quad((0, 6, 0), (8, 0, 0), (0, 0, 2.75), True)
    room.quad((3.25, 0, 0), (0, 4, 0), (0, 0, 2.75))  # partitions
    room.quad((3.25, 2.5, 0), (4.75, 0, 0), (0, 0, 2), True)
    room.quad((0.5, 4.5, 0), (2, 0, 0), (0, 0, 2.75))
    room.quad((1, 1, 1.125), (2, 0, 0), (0, 3, 0), True)  # a table top and a shelf board along the wall
    room.quad((0, 5.75, 1.5), (8, 0, 0), (0, 0.25, 0))
    cab = Builder()
    cab.box((0, 0, 0), (0.5, 0.75, 1.0), 0b010101)
    cab.box((1 / 64, 1 / 64, 1 / 64), (0.5 - 1 / 64, 0.75 - 1 / 64, 1 - 1 / 64), 0b101010)
    for k in range(3):  # (the shelves stop 1/64 short of the inner box: coincident faces are coplanar_panels' subject)
        cab.box((1 / 32, 1 / 32, 0.25 * (k + 1)), (0.5 - 1 / 32, 0.75 - 1 / 32, 0.25 * (k + 1) + 1 / 64), 0b110011 >> k)
    inst = [(MESH, 0, None)]
    for k in range(6):  # along the far wall, a hand's width apart and off the floor; two beside the door
        inst.append((MESH, 1, _translate(3.5 + 0.75 * k, 5.0, 0.25)))
    for k in range(2):
        inst.append((MESH, 1, _translate(0.25, 0.25 + 1.25 * k, 0.25)))
    for k in range(5):
        inst.append((MESH, 1, _translate(4.0 + 0.75 * k, 0.25, 1.5 if k % 2 else 0.25)))
    for k in range(6):
        inst.append((MESH, 1, _translate(0.25 + 1.25 * k, 3.0 + 0.25 * (k % 3), 1.25 if k % 2 else 0.25, 2.0 if k % 4 == 0 else 1.0)))
    return Scene("flat_room", [room.mesh(), cab.mesh()], inst, 101)


PANEL_OFFSETS = (0.0, "ulp", 1e-6, 1e-5, 1e-4)


def coplanar_panels():
    """cabinet fronts with a door in the SAME plane: per pair a box of size s in {1/2, 1, 2, 4} whose front face is one quad, and a door quad over its middle, displaced
    along the normal by 0, one float32 ulp of the plane's coordinate and 1e-6 of s (s = 1/2), 1e-5 and 1e-4 of s (every s) (1 / Q steps where that is representable, else written out in float32),
    triangulated along the OTHER diagonal; the front planes lie on a coordinate plane (c = 0) and off it, normal along x, y and z: three meshes, one per axis"""
    meshes, tiny = [], []
    for axis in range(3):
        bld = Builder()
        perm = [(axis + 1) % 3, (axis + 2) % 3, axis]  # local (a, b, normal) -> world axes
        n = 0
        for si, s in enumerate((0.5, 1.0, 2.0, 4.0)):
            col = 0
            for oi, off in enumerate(PANEL_OFFSETS[::-1]):  # (the larger offsets nearer the origin, where float32 still tells the two planes apart)
                for c in (0.0, 1.25 + 0.5 * si):
                    if (off == "ulp" and c == 0.0) or (off in PANEL_OFFSETS[:3] and s > 0.5):
                        continue  # (one ulp of 0 is no offset; the three smallest offsets -- below any t bar: undecided rays -- stay on the smallest size)
                    a0, b0 = 1.5 * s * col, (0.0, 1.0, 2.5, 5.0)[si]  # a row per size; the three meshes in different octants, clear of each other
                    if axis >= 1:
                        a0 = -a0 - s - 0.25
                    if axis == 2:
                        b0 = -b0 - s - 0.25
                    col += 1
                    if off in PANEL_OFFSETS[:3]:  # door and front of a pair no bar can tell apart: only the `overlap` rays are aimed at them
                        tiny += [21 * 14 * axis + 14 * n + q for q in (12, 13, 2 * (2 * axis + 1), 2 * (2 * axis + 1) + 1)]
                    n += 1
                    lo, hi = np.zeros(3), np.zeros(3)
                    lo[perm], hi[perm] = (a0, b0, c - 0.5 * s), (a0 + s, b0 + s, c)
                    bld.box(lo, hi, 0b000000 if n % 2 else 0b111111)
                    front_flip = bool(((0b000000 if n % 2 else 0b111111) >> (axis + 3)) & 1)
                    cc = float(np.nextafter(np.float32(c), np.float32(np.inf))) if off == "ulp" else float(np.float32(c + off * s))
                    p, eu, ev = np.zeros(3), np.zeros(3), np.zeros(3)
                    p[perm], eu[perm], ev[perm] = (a0 + 0.25 * s, b0 + 0.125 * s, cc), (0.5 * s, 0, 0), (0, 0.75 * s, 0)
                    bld.quad(p, eu, ev, not front_flip)
        assert n == 21
        meshes.append(bld.mesh())
    return Scene("coplanar_panels", meshes, [(MESH, g, None) for g in range(3)], 202, shares={"overlap": 0.008, "far": 0.03, "axis": 0.06, "grazing": 0.4, "surface": 0.005}, avoid=tiny)


def _rods(rods, segments=24):
    """a mesh per rod: the thinnest extent of its instance is the rod's diameter"""
    out = []
    for a, b, r in rods:
        bld = Builder()
        bld.cylinder(a, b, r, segments, phase=0.1)
        out.append(bld.mesh())
    return out


def slats():
    """24-facet cylinders and thin boards, 2 ... 10 long, facet width / board thickness such that the aspect runs from 50 : 1 to 500 : 1, along x and z beside a 12 x 3 wall
    (y = 0) over a floor"""
    wall = Builder()
    wall.quad((-1, 0, 0), (12, 0, 0), (0, 0, 3))
    wall.quad((-1, 0, 0), (0, 2, 0), (12, 0, 0), True)
    rods, boards = [], []
    k = 0
    for L in (2.0, 4.0, 8.0, 10.0):
        for aspect in (50.0, 150.0, 500.0):
            w = L / aspect
            r = w / (2 * np.sin(np.pi / 24))
            z = 0.25 + 0.2 * k
            rods.append(((0.0, 0.25 + 0.05 * (k % 4), z), (L, 0.25 + 0.05 * (k % 4), z), r))
            bd = Builder()
            bd.box((0.0, 0.75, z), (L, 0.75 + max(w, 1 / 256) * 4, z + max(_q(w), 1 / Q)), k)
            boards.append(bd.mesh())
            k += 1
    for i in range(8):  # uprights
        rods.append(((0.5 + 1.25 * i, 1.25, 0.0), (0.5 + 1.25 * i, 1.25, 3.0), 3.0 / (50.0 + 60.0 * i) / (2 * np.sin(np.pi / 24))))
    meshes = [wall.mesh()] + _rods(rods) + boards
    return Scene("slats", meshes, [(MESH, g, None) for g in range(len(meshes))], 303, rods=rods, shares={"silhouette": 0.005})


def mechanism_scene():
    """The architectural kitchen's rail whose facets record 865 fell between (docs/LOG.md): 24-facet rods 9.8 long of radius 0.0225 -- facets 0.006 wide, 1600 : 1 -- along x, y and z
    by a wall, seen from a few units away at 30 ... 45 degrees to the axis.  A ray that grazes a rod's silhouette meets two neighbouring facets almost in their
    planes: |det| << S, the weights' errors move the computed t by up to 3e-4 of t inside the facet's depth slab, hundreds of times the node test's 2^-19 slack, while the
    facet's box -- 0.006 thick across the ray -- starts behind that t.  Two such candidates are separated by more than the slack and by less than the intersector's error:
    which one a cull against the best t keeps depends on the visit order, i.e. on the tree."""
    wall = Builder()
    wall.quad((-5, 3.75, -4), (10, 0, 0), (0, 0, 8))
    wall.quad((-5, 0, -4), (0, 3.75, 0), (10, 0, 0), True)
    rods = []
    for k in range(16):  # every rod is a tube of two walls 2e-4 apart: behind each facet lies its twin, a second candidate within the first one's error
        if k < 6:  # along x in front of the wall, along y beside them, along z further out: each axis is the dominant one of the rays along its rods
            a, b = (-4.9, 3.25 + 0.0625 * (k % 3), -3.0 + 0.375 * k), (4.9, 3.25 + 0.0625 * (k % 3), -3.0 + 0.375 * k)
        elif k < 11:
            a, b = (-4.0 + 0.5 * (k - 6), -6.2, 0.375 * (k - 6)), (-4.0 + 0.5 * (k - 6), 3.6, 0.375 * (k - 6))
        else:
            a, b = (1.0 + 0.5 * (k - 11), 1.0 + 0.0625 * (k - 11), -3.9), (1.0 + 0.5 * (k - 11), 1.0 + 0.0625 * (k - 11), 5.9)
        rods += [(a, b, 0.0225), (a, b, 0.0223)]
    meshes = [wall.mesh()] + _rods(rods)
    return Scene("mechanism_scene", meshes, [(MESH, g, None) for g in range(len(meshes))], 404, rods=rods, shares={"silhouette": 0.009, "far": 0.03, "beside": 0.1, "axis": 0.06, "surface": 0.002, "edge": 0.001}, n_rays=20000,
                 avoid=np.arange(4, 4 + 48 * len(rods)))  # (a hit on a two-walled sliver tube is never decided: the general families aim at the wall, the random rays go anywhere)


SCENES = {"flat_room": flat_room, "coplanar_panels": coplanar_panels, "slats": slats, "mechanism_scene": mechanism_scene}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# world-space triangles and rays
# ---------------------------------------------------------------------------------------------------------------------------------------------
def world_triangles(arr):
    """-> instance, primitive, W (T, 3, 3) float64: the float32 vertices through the float32 matrix; the float32 evaluation in the checker's order gives the same numbers"""
    inst, prim, vid, M = hitref.triangle_table(arr)
    P = np.asarray(arr["vertices"]["pos"], np.float64)[vid]
    W = np.einsum("tij,tkj->tki", M[:, :, :3], P) + M[:, None, :, 3]
    P32, M32 = P.astype(np.float32), M.astype(np.float32)
    W32 = np.stack([((M32[:, a, 0, None] * P32[:, :, 0] + M32[:, a, 1, None] * P32[:, :, 1]) + M32[:, a, 2, None] * P32[:, :, 2]) + M32[:, a, 3, None] for a in range(3)], -1)
    assert np.array_equal(W32.astype(np.float64), W), "the scene's transforms are meant to be exact in float32"
    return inst, prim, W


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mk(o, d, tmin=0.0, tmax=1e16):
    r = np.zeros(len(o), S.RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, tmin, tmax
    return r


def _interior(rs, W, k, lo=0.1):
    w = rs.dirichlet((1.0, 1.0, 1.0), len(k)) * (1 - 3 * lo) + lo
    return np.einsum("nv,nvc->nc", w, W[k])


def _random_dirs(rs, n):
    return _unit(rs.normal(size=(n, 3)))


def make_rays(scene):
    """the closest-hit ray set of a scene (tmin 0, tmax 1e16), family by family; every family's share is a constant here"""
    arr = scene.arrays()
    inst, prim, W = world_triangles(arr)
    rs = np.random.RandomState(scene.seed)
    T = len(W)
    e = [W[:, 1] - W[:, 0], W[:, 2] - W[:, 1], W[:, 0] - W[:, 2]]
    nrm = _unit(np.cross(e[0], -e[2]))
    longest = np.max([np.linalg.norm(x, axis=1) for x in e], axis=0)
    lo, hi = W.reshape(-1, 3).min(0), W.reshape(-1, 3).max(0)
    # the thinnest extent of the instance a triangle belongs to (DESIGN.md's envelope is stated in it)
    thin = np.zeros(T)
    for i in np.unique(inst):
        ext = np.ptp(W[inst == i].reshape(-1, 3), axis=0)
        thin[inst == i] = ext.min()
    N = scene.n_rays
    out = []
    allowed = np.setdiff1d(np.arange(T), scene.avoid)

    aims = []

    def emit(k, r):
        """a family's rays and the world triangle each is aimed at (-1: none)"""
        out.append(r)
        aims.append(np.full(len(r), -1) if k is None else np.asarray(k))

    def pick(n, among=None):
        among = allowed if among is None else np.intersect1d(among, allowed)
        return among[rs.randint(0, len(among), n)]

    def count(share):
        return int(round(share * N))

    # (1) through shared edges and quad diagonals, exactly: a point on an edge, any direction
    n = count(scene.shares.get("edge", 0.004))
    k = rs.randint(0, T, n)
    ed = rs.randint(0, 3, n)
    a = W[k, ed]
    b = W[k, (ed + 1) % 3]
    p = a + rs.uniform(0.05, 0.95, (n, 1)) * (b - a)
    d = _random_dirs(rs, n)
    emit(k, _mk(p - d * rs.uniform(0.2, 2.0, (n, 1)), d))
    # (2) beside them: 1e-3 ... 1e-1 of the way into the triangle
    n = count(scene.shares.get("beside", 0.12))
    k = pick(n)
    ed = rs.randint(0, 3, n)
    a, b, c = W[k, ed], W[k, (ed + 1) % 3], W[k, (ed + 2) % 3]
    s = rs.uniform(0.05, 0.95, (n, 1))
    eps = 10.0 ** rs.uniform(-3, -1, (n, 1))
    p = (1 - eps) * (a + s * (b - a)) + eps * c
    d = _random_dirs(rs, n)
    emit(k, _mk(p - d * rs.uniform(0.2, 2.0, (n, 1)), d))
    # (3) grazing: 1e-3 ... 1e-1 rad to the plane of a triangle at least 1 long and 1/4 high, hit 0.05 ... 0.5 from the origin, its far vertex at least 10 times as far from the origin (a sliver seen along its plane has no bar: the silhouette rays below are those)
    n = count(scene.shares.get("grazing", 0.22))
    big = np.nonzero((longest >= 1.0) & (np.linalg.norm(np.cross(e[0], -e[2]), axis=1) / longest >= 0.25))[0]
    k = pick(n, big)
    p = _interior(rs, W, k)
    inplane = _unit(np.cross(nrm[k], _random_dirs(rs, n)))
    th = 10.0 ** rs.uniform(-3, -1, (n, 1))
    side = rs.choice([-1.0, 1.0], (n, 1))
    d = np.cos(th) * inplane - np.sin(th) * side * nrm[k]
    far = np.linalg.norm(W[k] - p[:, None, :], axis=2).max(axis=1)
    dist = np.minimum(rs.uniform(0.05, 0.5, n), far / 11.0)[:, None]  # (far is from the target: from the origin the far vertex is then >= 10 hit distances away)
    emit(k, _mk(p - d * dist, d))
    # (4) from far: 10 ... 1e3 thinnest instance extents (at most 100 units) from an interior target
    n = count(scene.shares.get("far", 0.2))
    k = pick(n)
    p = _interior(rs, W, k)
    d = _random_dirs(rs, n)
    dist = np.minimum(thin[k] * 10.0 ** rs.uniform(1, 3, n), 100.0)[:, None]
    emit(k, _mk(p - d * dist, d))
    # (5) axis-parallel, the other two components +0.0 / -0.0: at interior targets, and lying IN the planes of the axis-aligned quads
    n = count(scene.shares.get("axis", 0.12))
    k = pick(n)
    p = _interior(rs, W, k)
    ax = np.argmax(np.abs(nrm[k]), axis=1)
    inpl = rs.uniform(size=n) < 0.05
    ax = np.where(inpl, (ax + 1 + rs.randint(0, 2, n)) % 3, ax)
    d = np.where(rs.uniform(size=(n, 3)) < 0.5, 0.0, -0.0)
    d[np.arange(n), ax] = rs.choice([-1.0, 1.0], n)
    o = p - np.where(np.arange(3)[None, :] == ax[:, None], d, 0.0) * rs.uniform(0.1, 3.0, (n, 1))
    emit(k, _mk(o.astype(np.float32), d))
    # (6) origins ON a surface, tmin = 0 (the float32 point nearest to an interior one; exactly on it for the axis-aligned quads)
    n = count(scene.shares.get("surface", 0.01))
    k = pick(n)
    emit(k, _mk(_interior(rs, W, k).astype(np.float32), _random_dirs(rs, n)))
    # (7) a rod's silhouette: along one of its facets -- 30 ... 45 degrees to the axis (the axis is the ray's dominant one: the facet's depth slab is the rod's length) and, across it, 5e-4 ... 6e-3 rad to the facet's plane, from either side (from
    # inside the ray has come through the neighbouring facet a hair's breadth before) -- from 3 ... 8 units away
    n = count(scene.shares.get("silhouette", 0.0)) if scene.rods else 0
    if n:
        sliver = np.nonzero((inst >= 1) & (inst <= len(scene.rods)))[0]
        k = sliver[rs.randint(0, len(sliver), n)]
        axv = _unit(np.array([scene.rods[i - 1][1] for i in inst[k]], np.float64) - np.array([scene.rods[i - 1][0] for i in inst[k]], np.float64))
        across = _unit(np.cross(nrm[k], axv))
        ang = rs.uniform(np.pi / 6, np.pi / 4, (n, 1))
        phi = 10.0 ** rs.uniform(-3.3, -2.2, (n, 1)) * rs.choice([-1.0, 1.0], (n, 1))
        d = np.cos(ang) * axv * rs.choice([-1.0, 1.0], (n, 1)) + np.sin(ang) * (np.cos(phi) * across * rs.choice([-1.0, 1.0], (n, 1)) + np.sin(phi) * nrm[k])
        emit(k, _mk(_interior(rs, W, k, 0.02) - d * rs.uniform(3.0, 8.0, (n, 1)), d))
    # (8) into the overlap of a coplanar pair (the doors are the quads that follow each box: 12 triangles, then 2)
    n = count(scene.shares.get("overlap", 0.0))
    if n:
        doors = np.nonzero(prim % 14 >= 12)[0]
        k = doors[rs.randint(0, len(doors), n)]
        p = _interior(rs, W, k)
        d = _unit(-nrm[k] * rs.choice([-1.0, 1.0], (n, 1)) + 0.7 * _random_dirs(rs, n))
        emit(k, _mk(p - d * rs.uniform(0.3, 3.0, (n, 1)), d))
    # (9) the rest: anywhere inside the bounds, any direction
    n = N - sum(len(x) for x in out)
    emit(None, _mk(rs.uniform(lo - 0.5, hi + 0.5, (n, 3)), _random_dirs(rs, n)))
    rays = np.concatenate(out)
    assert len(rays) == N
    return rays, np.concatenate([np.full(len(x), i) for i, x in enumerate(out)]), np.concatenate(aims)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _perm_of(d):
    """make_shear's permutation of every direction: (kx, ky, kz)"""
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    kz = np.where(ax > ay, np.where(ax > az, 0, 2), np.where(ay > az, 1, 2))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = d[np.arange(len(d)), kz] < 0
    return np.stack([np.where(neg, ky, kx), np.where(neg, kx, ky), kz], 1)


def reference(rays, W, chunk=192):
    """the module docstring's bars and decisions for every ray against every triangle, in float64 on the float32 inputs widened exactly.  -> dict over the rays:
    tri (the certain nearest hit; -1: none), t, u, v, t_bar, b_bar, t_next (the nearest other triangle that may be hit), decided, hit (decided and hit)"""
    o_all, d_all = np.asarray(rays["origin"], np.float64), np.asarray(rays["dir"], np.float64)
    N, T = len(rays), len(W)
    res = {k: np.full(N, np.nan) for k in ("t", "u", "v", "t_bar", "b_bar", "t_next")}
    res["tri"] = np.full(N, -1, np.int64)
    res["decided"] = np.zeros(N, bool)
    perms = _perm_of(d_all)
    code = perms[:, 0] * 9 + perms[:, 1] * 3 + perms[:, 2]
    Lw = np.abs(W).max(axis=(1, 2))
    for cd in np.unique(code):
        sel = np.nonzero(code == cd)[0]
        pm = perms[sel[0]]
        Wp = W[:, :, pm]
        for s0 in range(0, len(sel), chunk):
            idx = sel[s0:s0 + chunk]
            o, d = o_all[idx][:, pm], d_all[idx][:, pm]
            Sz = 1.0 / d[:, 2]
            Sx, Sy = (d[:, 0] * Sz)[:, None], (d[:, 1] * Sz)[:, None]
            rel = Wp[None, :, :, :] - o[:, None, None, :]  # (n, T, vertex, xyz)
            zc = rel[..., 2]
            sx, sy = rel[..., 0] - Sx[..., None] * zc, rel[..., 1] - Sy[..., None] * zc
            X = (np.abs(rel[..., 0]) + np.abs(Sx[..., None] * zc)).max(axis=2)
            Y = (np.abs(rel[..., 1]) + np.abs(Sy[..., None] * zc)).max(axis=2)
            Ax, Bx, Cx = sx[..., 0], sx[..., 1], sx[..., 2]
            Ay, By, Cy = sy[..., 0], sy[..., 1], sy[..., 2]
            Uw, Vw, Ww = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
            det = (Uw + Vw) + Ww
            SX, SY = np.abs(sx).sum(axis=2), np.abs(sy).sum(axis=2)
            E = 3 * U * SX * SY + 10 * U * (X * SY + Y * SX)
            with np.errstate(divide="ignore", invalid="ignore"):
                cond = E / np.abs(det)
                z = zc * Sz[:, None, None]
                t = (Uw * z[..., 0] + Vw * z[..., 1] + Ww * z[..., 2]) / det
                zmax = np.abs(z).max(axis=2)
                nobar = ~(cond <= 0.25)
                zlo, zhi = z.min(axis=2), z.max(axis=2)
                b_bar = (2 * cond + 2 * U) / (1 - cond)
                L = np.maximum(Lw[None, :], np.abs(o).max(axis=1)[:, None])
                aSz = np.abs(Sz)[:, None]
                t_bar = (cond * np.abs(z - t[..., None]).max(axis=2) + 10 * U * zmax + U * (np.abs(Wp[None, :, :, 2]).max(axis=2) + np.abs(o[:, 2])[:, None]) * aSz +
                         hitref.C_ISECT * U * L * aSz * np.sqrt(3.0)) / (1 - cond)
                reject = 2.0 ** -20 * SX * SY * zmax / np.abs(det)
            # the sign test with every weight off by at most E: the ray may be inside / is inside for certain.  A pair without a bar may be hit anywhere in its depth slab
            wmin, wmax = np.minimum(np.minimum(Uw, Vw), Ww), np.maximum(np.maximum(Uw, Vw), Ww)
            near = (wmin > -E) | (wmax < E)
            maybe = near & np.where(nobar, zhi > 0, (t > -t_bar) & ~(np.abs(t) + t_bar < reject))  # (closer than its own error to the rejection threshold: rejected for certain)
            front = np.where(nobar, zlo, t - t_bar)
            sure = ~nobar & ((wmin > E) | (wmax < -E)) & (t > 2 * t_bar + reject)
            ts = np.where(sure, t, np.inf)
            k0 = np.argmin(ts, axis=1)
            r = np.arange(len(idx))
            t0 = ts[r, k0]
            found = np.isfinite(t0)
            fr = np.where(maybe, front, np.inf)
            fr[r, k0] = np.where(found, np.inf, fr[r, k0])
            nxt = fr.min(axis=1)
            tb0 = np.where(found, t_bar[r, k0], 0.0)
            decided = np.where(found, nxt > t0 + tb0, ~maybe.any(axis=1))
            tn = np.where(maybe, np.where(nobar, zlo, t), np.inf)
            tn[r, k0] = np.where(found, np.inf, tn[r, k0])
            res["tri"][idx] = np.where(found, k0, -1)
            res["t"][idx] = np.where(found, t0, np.nan)
            res["u"][idx] = np.where(found, Vw[r, k0] / np.where(found, det[r, k0], 1.0), np.nan)
            res["v"][idx] = np.where(found, Ww[r, k0] / np.where(found, det[r, k0], 1.0), np.nan)
            res["t_bar"][idx] = np.where(found, t_bar[r, k0], np.nan)
            res["b_bar"][idx] = np.where(found, b_bar[r, k0], np.nan)
            res["t_next"][idx] = tn.min(axis=1)
            res["decided"][idx] = decided
    res["hit"] = res["decided"] & (res["tri"] >= 0)
    return res


def shadow_twins(rays, ref, every=3):
    """any-hit twins of every `every`-th decided hit: the same ray with tmax just short of the hit and just past it, at 2^-22, 2^-18 and 2^-14 of t -- inside the
    intersector's error, at the node test's slack, and clear of both"""
    k = np.nonzero(ref["hit"])[0][::every]
    out = []
    for j, rel in enumerate((2.0 ** -22, 2.0 ** -18, 2.0 ** -14)):
        for sign in (-1.0, 1.0):
            r = rays[k[j::3]].copy()
            r["tmax"] = (ref["t"][k[j::3]] * (1.0 + sign * rel)).astype(np.float32)
            out.append(r)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def cached(name):
    """-> scene, its arrays, (instance, primitive, W), the closest-hit rays, the reference, the any-hit twins: built once per process and never written to"""
    scene = SCENES[name]()
    arr = scene.arrays()
    tri = world_triangles(arr)
    rays, family, aim = make_rays(scene)
    # TREEREF_CACHE: a directory a parent process keeps the reference in for the child processes it starts (tests/test_gpu_tree_independence.py: 40 s of numpy once)
    path = os.path.join(os.environ["TREEREF_CACHE"], name + ".npz") if os.environ.get("TREEREF_CACHE") else None
    if path and os.path.exists(path):
        with np.load(path) as z:
            assert np.array_equal(z["rays"], rays.view(np.uint8)), "the cached reference belongs to other rays"
            ref = {k[4:]: z[k] for k in z.files if k.startswith("ref_")}
    else:
        ref = reference(rays, tri[2])
        ref["family"], ref["aim"] = family, aim
    shadow = shadow_twins(rays, ref)
    for a in (rays, shadow, tri[0], tri[1], tri[2], *ref.values()):
        a.setflags(write=False)
    return scene, arr, tri, rays, ref, shadow


def export(name, directory):
    """write a scene's reference where a child process started with TREEREF_CACHE=directory finds it"""
    scene, arr, tri, rays, ref, shadow = cached(name)
    path = os.path.join(str(directory), name + ".npz")
    if not os.path.exists(path):
        np.savez(path + ".tmp.npz", rays=rays.view(np.uint8), **{"ref_" + k: v for k, v in ref.items()})
        os.replace(path + ".tmp.npz", path)


def shares(name):
    """(undecided share, hit share) of a scene's rays: hit = decided and hit"""
    ref = cached(name)[4]
    return 1.0 - float(ref["decided"].mean()), float(ref["hit"].mean())


def check_decided(name, hits):
    """hit records against the reference on the decided rays: the float64 primitive exactly (a miss where it says so), t, u, v inside the bars.
    -> (rays naming another primitive, worst fraction of the t bar, of the barycentric bar)"""
    scene, arr, (inst, prim, W), rays, ref, shadow = cached(name)
    d, h = ref["decided"], ref["hit"]
    k = np.where(h, ref["tri"], 0)
    want_inst, want_prim = np.where(h, inst[k], 0xFFFFFFFF), np.where(h, prim[k], 0xFFFFFFFF)
    wrong = d & ((hits["instance_id"] != want_inst) | (hits["prim_id"] != want_prim))
    ok = h & ~wrong
    ft = np.abs(hits["t"].astype(np.float64) - ref["t"])[ok] / ref["t_bar"][ok]
    fb = np.maximum(np.abs(hits["u"].astype(np.float64) - ref["u"]), np.abs(hits["v"].astype(np.float64) - ref["v"]))[ok] / ref["b_bar"][ok]
    return np.nonzero(wrong)[0], float(ft.max()), float(fb.max())
