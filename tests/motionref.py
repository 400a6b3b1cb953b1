"""Object motion's definition (include/strelka_hip.h, "Object motion") in numpy: skh_rewind_guides twice, and the table's derivation.

rewind32   the definition restated operation by operation in float32.  It has + - x /, one square root, compare and select, each of which numpy's float32 rounds
           as IEEE 754 says -- as the device does with contraction off and its correctly rounded division and square root.  The device must give these bits.

rewind64   the same definition in float64 on the same float32 words, with a per-word error bar for the float32 evaluation that is a written-out count of roundings,
           as tests/temporalref.py does it.  u = 2^-24 is float32's unit roundoff.
             P*.x   ((m0 P.x + m1 P.y) + m2 P.z) + m3: three products (u each of its own magnitude) and three additions whose partial sums are at most
                    D = |m0 P.x| + |m1 P.y| + |m2 P.z| + |m3| (u D each): 4 u D, one u D spare: 5 u D
             v.x    (k0 N.x + k1 N.y) + k2 N.z: three products and two additions, Dv = |k0 N.x| + |k1 N.y| + |k2 N.z|: 3 u Dv, one spare: ev = 4 u Dv
             s      (v.x v.x + v.y v.y) + v.z v.z: each square carries 2 |v| ev from its operand and u v^2 of the product, the two additions u s each, one
                    spare: es = sum 2 |v_k| ev_k + 4 u s
             r      sqrtf(s): es / (2 r) from its operand and u r of the root: er = es / (2 r) + u r
             N*.x   v.x / r: ev.x / r from the numerator, |v.x| er / r^2 from the denominator, u |N*.x| of the quotient, one spare:
                    ev.x / r + |v.x| er / r^2 + 2 u |N*.x|
           (first order in u; the inputs the tests use keep s well away from the cancellation where second-order terms would count.)
           The decisions -- kind, instance_id < n, the flag bits -- read input words: they have no rounding and no margin, so no pixel is ambiguous.  A copied
           word, a DROP position and a .w word are exact: bar 0, and the comparison is of bits.

motion64   the table's derivation through np.linalg: to_prev = A B^-1 as a 3 x 4, normal_to_prev = its linear part's inverse transpose.

synthetic  a two-frame input at 67 x 45 after temporalref.synthetic's, with the box and the sphere as instances of their own that moved between the frames."""
import numpy as np

from tests import temporalref as T

U = 2.0 ** -24
MOVED, DROP = 1, 2
QNAN = np.uint32(0x7FC00000)
ENTRY = np.dtype([("to_prev", np.float32, 12), ("normal_to_prev", np.float32, 9), ("flags", np.uint32), ("reserved", np.uint32, 2)])
assert ENTRY.itemsize == 96


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_words(got, want):
    """word for word: the same bits, or a NaN where the restatement has a NaN -- the payload of a NaN that an OPERATION produced is no part of the definition (a
    NaN that is copied keeps its bits: check() compares those words as bits)"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all())


def entry(to_prev=None, normal_to_prev=None, flags=0):
    e = np.zeros((), ENTRY)
    e["to_prev"] = np.eye(3, 4).reshape(12) if to_prev is None else np.asarray(to_prev, np.float64).reshape(12)
    e["normal_to_prev"] = np.eye(3).reshape(9) if normal_to_prev is None else np.asarray(normal_to_prev, np.float64).reshape(9)
    e["flags"] = flags
    return e


def motion64(prev, cur):
    """`prev`, `cur`: an instance's 3 x 4 row-major transforms (12 words) -> (to_prev 3 x 4, normal_to_prev 3 x 3), float64"""
    A, B = np.eye(4), np.eye(4)
    A[:3], B[:3] = np.asarray(prev, np.float64).reshape(3, 4), np.asarray(cur, np.float64).reshape(3, 4)
    X = A @ np.linalg.inv(B)
    return X[:3], np.linalg.inv(X[:3, :3]).T


def table_from(prev_transforms, cur_transforms):
    """the table of a list of transform pairs, through motion64 rounded once; equal words give flags 0"""
    t = np.zeros(len(cur_transforms), ENTRY)
    for i, (a, b) in enumerate(zip(prev_transforms, cur_transforms)):
        a, b = np.asarray(a, np.float32).reshape(12), np.asarray(b, np.float32).reshape(12)
        if np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            t[i] = entry()
        else:
            t[i] = entry(*motion64(a, b), flags=MOVED)
    return t


def _select(ids, table):
    """per pixel: the clamped entry, `applies`, `drop`"""
    ids, table = np.asarray(ids, np.uint32), np.asarray(table, ENTRY).reshape(-1)
    n = len(table)
    inst, kind = ids[..., 0], ids[..., 3]
    e = table[np.minimum(inst, n - 1)]
    applies = ((kind == 1) | (kind == 2)) & (inst < n) & ((e["flags"] & MOVED) != 0)
    return e, applies, applies & ((e["flags"] & DROP) != 0)


def rewind32(ids, position, normal, table):
    """the definition in float32.  Planes (h, w, 4) as the device gets them, `table` an ENTRY array with n >= 1 -> {"position", "normal"}, (h, w, 4) float32"""
    f = np.float32
    P, N = np.ascontiguousarray(position, f), np.ascontiguousarray(normal, f)
    e, applies, drop = _select(ids, table)
    m, k = e["to_prev"].astype(f), e["normal_to_prev"].astype(f)
    with np.errstate(all="ignore"):
        Ps = [((m[..., 4 * r] * P[..., 0] + m[..., 4 * r + 1] * P[..., 1]) + m[..., 4 * r + 2] * P[..., 2]) + m[..., 4 * r + 3] for r in range(3)]
        v = [(k[..., 3 * r] * N[..., 0] + k[..., 3 * r + 1] * N[..., 1]) + k[..., 3 * r + 2] * N[..., 2] for r in range(3)]
        s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        root = np.sqrt(s)
        Ns = [v[r] / root for r in range(3)]
    po, no = bits(P).copy(), bits(N).copy()
    moved = applies & ~drop
    for r in range(3):
        po[..., r] = np.where(applies, np.where(drop, QNAN, bits(Ps[r].astype(f))), po[..., r])
        no[..., r] = np.where(moved, bits(Ns[r].astype(f)), no[..., r])
    return {"position": po.view(f), "normal": no.view(f)}


def rewind64(ids, position, normal, table):
    """the definition in float64 on the float32 words -> {"position", "normal": (h, w, 4) float64, "bar_position", "bar_normal": (h, w, 4),
    "exact_position", "exact_normal": (h, w, 4) bool -- words that are copies or constants and are compared as bits with "bits_position" / "bits_normal",
    "applies", "drop": (h, w) bool}"""
    f, d = np.float32, np.float64
    P32, N32 = np.ascontiguousarray(position, f), np.ascontiguousarray(normal, f)
    P, N = P32.astype(d), N32.astype(d)
    e, applies, drop = _select(ids, table)
    m, k = e["to_prev"].astype(d), e["normal_to_prev"].astype(d)
    moved = applies & ~drop
    pos, nrm = P.copy(), N.copy()
    bp, bn = np.zeros(P.shape), np.zeros(N.shape)
    with np.errstate(all="ignore"):
        v, ev = [], []
        for r in range(3):
            terms = [m[..., 4 * r] * P[..., 0], m[..., 4 * r + 1] * P[..., 1], m[..., 4 * r + 2] * P[..., 2], m[..., 4 * r + 3]]
            pos[..., r] = np.where(moved, terms[0] + terms[1] + terms[2] + terms[3], pos[..., r])
            bp[..., r] = np.where(moved, 5 * U * sum(np.abs(t) for t in terms), 0.0)
            nt = [k[..., 3 * r] * N[..., 0], k[..., 3 * r + 1] * N[..., 1], k[..., 3 * r + 2] * N[..., 2]]
            v.append(nt[0] + nt[1] + nt[2])
            ev.append(4 * U * sum(np.abs(t) for t in nt))
        s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        es = sum(2 * np.abs(v[r]) * ev[r] for r in range(3)) + 4 * U * s
        root = np.sqrt(s)
        er = es / (2 * root) + U * root
        for r in range(3):
            q = v[r] / root
            nrm[..., r] = np.where(moved, q, nrm[..., r])
            bn[..., r] = np.where(moved, ev[r] / root + np.abs(v[r]) * er / (root * root) + 2 * U * np.abs(q), 0.0)
    pos[drop, :3] = np.nan
    exact_p, exact_n = np.ones(P.shape, bool), np.ones(N.shape, bool)
    exact_p[..., :3] = ~moved[..., None]
    exact_n[..., :3] = ~moved[..., None]
    bits_p, bits_n = bits(P32).copy(), bits(N32).copy()
    bits_p[drop, :3] = QNAN
    return {"position": pos, "normal": nrm, "bar_position": bp, "bar_normal": bn, "exact_position": exact_p, "exact_normal": exact_n,
            "bits_position": bits_p, "bits_normal": bits_n, "applies": applies, "drop": drop}


def check(got, ref):
    """`got`: {"position", "normal"} float32.  Asserts the exact words bit for bit and returns the worst |got - ref| / bar over every other word of every pixel (a
    word whose reference is NaN must be NaN; 0 where both are equal)"""
    worst = 0.0
    for name in ("position", "normal"):
        g32 = np.ascontiguousarray(got[name], np.float32)
        exact = ref["exact_" + name]
        assert np.array_equal(bits(g32)[exact], ref["bits_" + name][exact]), f"a copied or constant word of {name} differs"
        g, want, bar = g32.astype(np.float64)[~exact], ref[name][~exact], ref["bar_" + name][~exact]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan), f"NaN words of {name} differ"
        with np.errstate(invalid="ignore"):
            err = np.where(g == want, 0.0, np.abs(g - want))[~nan]  # (an infinity that both have is no error; one that only one has is an infinite one)
        assert not np.isnan(err).any()
        ratio = np.where(err == 0.0, 0.0, err / np.where(bar[~nan] > 0.0, bar[~nan], np.finfo(np.float64).tiny))
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the synthetic input
# ---------------------------------------------------------------------------------------------------------------------------------------------
BOX_HALF = np.array([0.6, 0.6, 0.5])   # the box in its own space: centred on the origin
SPHERE_RADIUS = 0.6                     # the sphere in its own space: about the origin
BOX_AT, SPHERE_AT = np.array([-1.0, 0.6, -2.1]), np.array([0.9, 0.6, -1.8])
N_INSTANCES = 5                         # floor 0, wall 1, box 2, sphere 3, and an entry 4 no pixel has


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pose(at, axis=(0, 1, 0), degrees=0.0, scale=(1, 1, 1), shift=(0, 0, 0)):
    """an instance transform as 12 float32 words: scale, then rotation, about the object's origin; then the translation at + shift"""
    M = np.zeros((3, 4))
    M[:, :3] = _rotation(axis, degrees) @ np.diag(np.asarray(scale, np.float64))
    M[:, 3] = np.asarray(at, np.float64) + np.asarray(shift, np.float64)
    return M.astype(np.float32).reshape(12)


# the poses of the previous and of the current frame: a rotation, a non-uniform scale in [0.6, 1.4] and a translation carry each object from one to the other
POSES_PREV = {"box": pose(BOX_AT), "sphere": pose(SPHERE_AT)}
POSES_NOW = {"box": pose(BOX_AT, (0.1, 1.0, 0.05), 14.0, (1.15, 0.8, 0.9), (0.22, -0.12, 0.15)),
             "sphere": pose(SPHERE_AT, (0.3, 1.0, 0.2), 25.0, (0.75, 1.25, 1.1), (-0.3, 0.2, 0.28))}


def cast(cam, width, height, poses):
    """temporalref.cast with the box (instance 2) and the sphere (instance 3, kind 2) under the instance transforms `poses`: the ray is taken into the object's
    space, the hit's normal back with the inverse transpose -> ids uint32, normal, position, albedo float32, (h, w, 4) each"""
    eye, right, up, fwd, tx, ty = cam
    h, w = height, width
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b = (xx + 0.5) / w * 2 - 1, (yy + 0.5) / h * 2 - 1
    D = fwd + (a * tx)[..., None] * right + (b * ty)[..., None] * up
    t = np.full((h, w), np.inf)
    inst = np.full((h, w), -1)
    Nn = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        def take(tc, ok, i, n):
            nonlocal t, inst, Nn
            ok = ok & (tc > 1e-9) & (tc < t)
            t, inst = np.where(ok, tc, t), np.where(ok, i, inst)
            Nn = np.where(ok[..., None], n, Nn)

        tf = -eye[1] / D[..., 1]
        take(tf, np.isfinite(tf), 0, np.array([0.0, 1.0, 0.0]))
        tw = (T.WALL_Z - eye[2]) / D[..., 2]
        yw = eye[1] + tw * D[..., 1]
        take(tw, np.isfinite(tw) & (yw >= 0) & (yw <= T.WALL_TOP), 1, np.array([0.0, 0.0, 1.0]))

        def local(name):
            M = np.asarray(poses[name], np.float64).reshape(3, 4)
            inv = np.linalg.inv(M[:, :3])
            return (eye - M[:, 3]) @ inv.T, D @ inv.T, inv.T  # (origin, direction, and what takes an object-space normal to a world one, unnormalised)

        def world_normal(n_obj, to_world):
            n = n_obj @ to_world.T
            return n / np.linalg.norm(n, axis=-1, keepdims=True)

        o, d, nt = local("box")
        t0, t1 = (-BOX_HALF - o) / d, (BOX_HALF - o) / d
        tn, tfar = np.minimum(t0, t1), np.maximum(t0, t1)
        tin, tout = tn.max(-1), tfar.min(-1)
        ax = tn.argmax(-1)
        nb = np.zeros((h, w, 3))
        for k in range(3):
            nb[..., k] = np.where(ax == k, -np.sign(d[..., k]), 0.0)
        take(tin, tin <= tout, 2, world_normal(nb, nt))
        o, d, nt = local("sphere")
        A, B, Cq = (d * d).sum(-1), 2 * (d * o).sum(-1), (o * o).sum() - SPHERE_RADIUS ** 2
        disc = B * B - 4 * A * Cq
        ts = (-B - np.sqrt(disc)) / (2 * A)
        take(ts, disc > 0, 3, world_normal((o + ts[..., None] * d) / SPHERE_RADIUS, nt))
    hit = inst >= 0
    Pw = np.where(hit[..., None], eye + np.where(hit, t, 0.0)[..., None] * D, 0.0)
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 0] = np.where(hit, inst, 0xFFFFFFFF)
    ids[..., 1] = np.where(hit, 0, 0xFFFFFFFF)
    ids[..., 2] = np.where(hit, inst, 0xFFFFFFFF)
    ids[..., 3] = np.where(hit, np.where(inst == 3, 2, 1), 0)
    Nf, Pf, Af = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    Nf[..., :3], Nf[..., 3] = Nn, np.where(hit, 1.0, 0.0)
    Pf[..., :3], Pf[..., 3] = Pw, np.where(hit, 1.0, 0.0)
    Af[..., :3], Af[..., 3] = np.where(hit[..., None], T.ALBEDOS[np.clip(inst, 0, 3)], 0.0), np.where(hit, 1.0, 0.0)
    return ids, Nf, Pf, Af


def synthetic(width=67, height=45, seed=7):
    """two cameras a step apart over temporalref's scene, the box and the sphere in POSES_PREV for the previous frame and in POSES_NOW for the current one.
    -> temporalref.synthetic's dictionary ({"color", "ids", "normal", "position", "albedo"}, "prev", "matrix", "params"), and "table": the ENTRY table of the
    N_INSTANCES instances -- the floor unmoved (flags 0), the wall MOVED | DROP, the box and the sphere MOVED, entry 4 MOVED with no pixel -- "transforms":
    (previous, current) lists of 12 words per instance, "moved": (h, w) bool, the box's and the sphere's pixels.
    Planted in the current IDS: a miss rectangle (instance_id 0xffffffff), a kind-3 rectangle, a surface rectangle on the box with the instance id 7 >= n."""
    rs = np.random.RandomState(seed)
    h, w = height, width
    aspect = w / float(h)
    cam_prev = T.camera((0.0, 1.2, 2.0), (0.0, 0.6, -2.0), 55.0, aspect)
    cam_now = T.camera((0.35, 1.35, 1.9), (-0.1, 0.55, -2.0), 55.0, aspect)
    ids, N, P, A = cast(cam_now, w, h, POSES_NOW)
    pids, pN, pP, pA = cast(cam_prev, w, h, POSES_PREV)
    moved = (ids[..., 3] != 0) & ((ids[..., 0] == 2) | (ids[..., 0] == 3))
    T.plant(ids, N, P, A, (h // 2, h // 2 + 3, 4, 12), 0)
    T.plant(ids, N, P, A, (h // 2 + 5, h // 2 + 8, w - 14, w - 6), 3)
    T.plant(pids, pN, pP, pA, (h - 8, h - 5, w // 2, w // 2 + 7), 0)
    by, bx = np.nonzero((ids[..., 0] == 2) & (ids[..., 3] == 1))
    cy, cx = int(np.median(by)), int(np.median(bx))
    ids[cy:cy + 2, cx:cx + 3, 0] = 7  # (surface pixels of an instance the table does not have)
    moved &= (ids[..., 3] == 1) | (ids[..., 3] == 2)
    moved &= ids[..., 0] < N_INSTANCES
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    irr = 0.6 + 0.3 * np.sin(xx * 0.11) * np.cos(yy * 0.07)
    C = np.zeros((h, w, 4), np.float32)
    C[..., :3] = A[..., :3] * (irr[..., None] + rs.uniform(-0.4, 0.4, (h, w, 3)))
    C[..., 3] = rs.uniform(0.0, 1.0, (h, w))
    C[ids[..., 3] == 3, :3] = 40.0
    Hs = np.zeros((h, w, 4), np.float32)
    Hs[..., :3] = irr[..., None] + rs.uniform(-0.2, 0.2, (h, w, 3))
    Hs[..., 3] = rs.choice([1.0, 2.0, 5.0, 17.5, 32.0, 8.0], size=(h, w))
    psurf = (pids[..., 3] == 1) | (pids[..., 3] == 2)
    Hs[~psurf] = 0.0
    identity = pose((0, 0, 0))
    prev_t = [identity, identity, POSES_PREV["box"], POSES_PREV["sphere"], pose((0, 0, 0))]
    cur_t = [identity, identity, POSES_NOW["box"], POSES_NOW["sphere"], pose((0, 0, 0), (1, 0, 0), 90.0, shift=(1, 2, 3))]
    table = table_from(prev_t, cur_t)
    table[1]["flags"] = MOVED | DROP
    M = T.world_to_clip(cam_prev)
    return {"color": C, "ids": ids, "normal": N, "position": P, "albedo": A, "prev": {"history": Hs, "ids": pids, "normal": pN, "position": pP}, "matrix": M,
            "params": T.params(w, h, M), "table": table, "transforms": (prev_t, cur_t), "moved": moved}
