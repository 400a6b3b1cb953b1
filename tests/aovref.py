"""The first-hit AOV planes ("First-hit AOVs"; include/strelka_hip.h: skh_render_aovs) restated in numpy: what the planes of a list of
rays must hold, given the rays, their hit records (t, instance_id, prim_id, u, v) and the flat scene arrays.  numpy only.

  ids       instance_id, prim_id, material, kind: assembled exactly from the records and the instance table
  hit       t, u, v: the records' own; depth: float64, from a given position
  P, N, Ng  float64, from tests/hitref.py: triangle_state at the records' barycentrics (the mapped normal where the material has a normal map), curve_state at
            origin + t direction, origin + t direction itself for a light proxy

U = 2^-24, as in hitref.  The one bound this file adds is depth_bound; its docstring is the derivation."""
import numpy as np

from tests import hitref

U = hitref.U
MISS = 0xFFFFFFFF
KIND_MISS, KIND_TRIANGLE, KIND_CURVE, KIND_LIGHT = 0, 1, 2, 3
PLANES = ("ids", "hit", "normal", "position", "geom_normal", "albedo", "texcoord")


def material_index(arr, inst):
    """the index k_shade resolves for the instances `inst`: 0xffffffff -> 0, beyond the list -> 0"""
    m = np.asarray(arr["instances"]["material_id"], np.int64)[inst]
    return np.where((m == MISS) | (m >= len(arr["materials"])), 0, m)


def ids_and_hit(arr, rec):
    """-> (ids (N, 4) uint32, thit (N, 3) float32): exact.  A miss is instance 0xffffffff: ids 0xffffffff, 0xffffffff, 0xffffffff, 0 and t = -1, u = v = 0."""
    inst = np.asarray(rec["instance_id"], np.uint32)
    miss = inst == MISS
    safe = np.where(miss, 0, inst).astype(np.int64)
    typ = np.asarray(arr["instances"]["type"], np.int64)[safe]
    kind = np.where(miss, KIND_MISS, np.where(typ == 0, KIND_TRIANGLE, np.where(typ == 2, KIND_CURVE, KIND_LIGHT)))
    mat = np.where((kind == KIND_TRIANGLE) | (kind == KIND_CURVE), material_index(arr, safe), MISS)
    ids = np.stack([np.where(miss, MISS, inst), np.where(miss, MISS, np.asarray(rec["prim_id"], np.uint32)), mat, kind], 1).astype(np.uint32)
    thit = np.stack([np.where(miss, np.float32(-1), rec["t"]), np.where(miss, np.float32(0), rec["u"]), np.where(miss, np.float32(0), rec["v"])], 1).astype(np.float32)
    return ids, thit


def depth64(world_to_clip, P):
    """clip = world_to_clip (P, 1), depth = clip.z / clip.w in float64; world_to_clip the 16 float32 words of the parameters (row-major), P (N, 3), both widened exactly
    -> (depth, S_z, S_w, w): S = sum |m_k p_k| of the z and of the w row"""
    M = np.asarray(world_to_clip, np.float32).astype(np.float64).reshape(4, 4)
    p = np.concatenate([np.asarray(P, np.float64).reshape(-1, 3), np.ones((len(np.asarray(P).reshape(-1, 3)), 1))], 1)
    z, w = p @ M[2], p @ M[3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return z / w, np.abs(p * M[2]).sum(1), np.abs(p * M[3]).sum(1), w


def depth_bound(world_to_clip, P):
    """|device depth - depth64| for the plane's OWN float32 position P as the input (exact in both).
      a row of mul44, ((m0 x + m1 y) + m2 z) + m3 1: four products and three sums, each rounded once, each on a partial result no larger than S = sum |m_k p_k|:
        7 U S absolute, for the z row and for the w row;
      the quotient z' / w' of the rounded rows: z' / w' - z / w = (dz - (z / w) dw) / w', |w'| >= |w| - 7 U S_w: (7 U S_z + |depth| 7 U S_w) / (|w| - 7 U S_w);
      the division rounds once: U of the quotient it found, |depth| + the line above.
    -> (bound, depth64)"""
    d, sz, sw, w = depth64(world_to_clip, P)
    q = (7 * U * sz + np.abs(d) * 7 * U * sw) / (np.abs(w) - 7 * U * sw)
    return q + U * (np.abs(d) + q), d


def triangle_hit(arr, rec, origin, direction, sel):
    """the records of the rays `sel` (all triangle hits) as a hitref.first_hits dict: `tri` from (instance, primitive), `bary` = the records' fp32 barycentrics"""
    inst, prim, vid, M = hitref.triangle_table(arr)
    key = {(int(i), int(p)): k for k, (i, p) in enumerate(zip(inst, prim))}
    n = len(rec)
    tri = np.full(n, -1, np.int64)
    for i in np.nonzero(sel)[0]:
        tri[i] = key[(int(rec["instance_id"][i]), int(rec["prim_id"][i]))]
    return {"tri": tri, "bary": np.stack([rec["u"], rec["v"]], 1).astype(np.float64), "origin": np.asarray(origin, np.float64).reshape(-1, 3),
            "dir": np.asarray(direction, np.float64).reshape(-1, 3)}


def normal_texel(arr, material):
    """the constant (r, g, b) bytes of a material's normal map, or None without one (the scenes of tests/test_hit_cpu.py use constant maps)"""
    t = int(arr["materials"]["normal_texture"][material])
    if t == 0 or t > len(arr.get("textures") or []):
        return None
    tex = np.asarray(arr["textures"][t - 1])
    assert (tex == tex[0, 0]).all(), "a constant normal map"
    return tuple(int(x) for x in tex[0, 0, :3])


def assemble(arr, origin, direction, rec, world_to_clip=None):
    """the expected planes of N rays (origin, direction: (N, 3) float32; rec: N hit records) -> dict: ids (N, 4) uint32 and hit (N, 3) float32, exact; position,
    normal, geom_normal (N, 3) float64 (0 at a miss; a light proxy: position only) and facing (N,); with world_to_clip, depth (N,) float64 of the float64 position
    (1 at a miss).  Albedo and texture coordinates are held to the device's own probe and to mtexref by the tests that check them."""
    o, d = np.asarray(origin, np.float64).reshape(-1, 3), np.asarray(direction, np.float64).reshape(-1, 3)
    ids, thit = ids_and_hit(arr, rec)
    kind = ids[:, 3]
    n = len(ids)
    P, N, Ng, facing = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    tri = kind == KIND_TRIANGLE
    if tri.any():
        h = triangle_hit(arr, rec, o, d, tri)
        for m in np.unique(ids[tri, 2]):  # (the normal map is the material's)
            s = tri & (ids[:, 2] == m)
            texel = normal_texel(arr, int(m))
            st = hitref.triangle_state(arr, {**h, "tri": np.where(s, h["tri"], -1)}, texel)
            P[s], Ng[s], N[s] = st["position"][s], st["geom_normal"][s], (st["normal"] if texel is None else st["mapped"])[s]
    cur = kind == KIND_CURVE
    pt = o + np.asarray(rec["t"], np.float64)[:, None] * d
    for i in np.unique(ids[cur, 0]):
        s = cur & (ids[:, 0] == i)
        cs = hitref.curve_state(arr, int(i), ids[s, 1].astype(np.int64), pt[s])
        P[s], N[s], Ng[s] = pt[s], cs["normal"], cs["normal"]
    lit = kind == KIND_LIGHT
    P[lit] = pt[lit]
    surf = tri | cur
    facing[surf] = np.where((Ng[surf] * -d[surf]).sum(1) >= 0, 1.0, -1.0)
    out = {"ids": ids, "hit": thit, "position": P, "normal": N, "geom_normal": Ng, "facing": facing}
    if world_to_clip is not None:
        dep = depth64(world_to_clip, P)[0]
        out["depth"] = np.where(kind == KIND_MISS, 1.0, dep)
    return out


def normals_view(normal, kind):
    """what the `debug = 1` view shows for a NORMAL plane: (N + 1) / 2 in float32 on surfaces (kinds 1 and 2), black elsewhere -- a miss is black in the view, and a
    light proxy shows the light, not a normal"""
    n = np.asarray(normal, np.float32)[..., :3]
    img = (n + np.float32(1.0)) * np.float32(0.5)
    k = np.asarray(kind)
    return np.where(((k == KIND_TRIANGLE) | (k == KIND_CURVE))[..., None], img, np.float32(0.0)).astype(np.float32)
