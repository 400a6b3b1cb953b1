"""Object motion off the GPU ("Object motion"): the ABI's symbols and the record's layout through the C compiler;
skh_instance_motion_check's table of refusals; skh_instance_motion_from_transforms against numpy's linear algebra; the float32 restatement of skh_rewind_guides
(tests/motionref.py: rewind32) inside the float64 reference's written-out bar and against closed forms; the conditions the synthetic two-frame input must meet,
and what the rewound planes do to temporalref's reprojection of it.  No test here needs a GPU; every one that touches the library fails without the feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import motionref as M
from tests import temporalref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IDENTITY = np.eye(3, 4).astype(f32).reshape(12)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


@pytest.fixture(scope="module")
def syn():
    return M.synthetic()


def derive(prev, cur):
    """skh_instance_motion_from_transforms on two 12-word transforms -> an S.INSTANCE_MOTION record"""
    a, b = np.ascontiguousarray(prev, f32).reshape(12), np.ascontiguousarray(cur, f32).reshape(12)
    e = np.zeros((), S.INSTANCE_MOTION)
    assert capi.load().skh_instance_motion_from_transforms(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p)) == 0
    return e


def transform(linear, t=(0, 0, 0)):
    X = np.zeros((3, 4))
    X[:, :3], X[:, 3] = linear, t
    return X.astype(f32).reshape(12)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# header <-> library <-> binding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_instance_motion_from_transforms", "skh_instance_motion_check", "skh_set_instance_motion", "skh_rewind_guides", "skh_get_rewind_info"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("set_instance_motion", "rewind_guides_device", "rewind_guides", "rewind_info"):
        assert callable(getattr(capi.Context, method))
    dt = S.INSTANCE_MOTION
    fields = ("to_prev", "normal_to_prev", "flags", "reserved")
    assert dt.itemsize == 96 and dt.names == fields and [dt.fields[n][1] for n in fields] == [0, 48, 84, 88]
    assert M.ENTRY == dt and (S.MOTION_MOVED, S.MOTION_DROP) == (1, 2) == (M.MOVED, M.DROP)
    info = ("calls", "pixels", "ms_last", "entries")
    assert capi.REWIND_INFO.itemsize == 32 and capi.REWIND_INFO.names == info and [capi.REWIND_INFO.fields[n][1] for n in info] == [0, 8, 16, 24]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu", sizeof(skh_instance_motion), sizeof(skh_rewind_info));\n'
                   + "".join(f'printf(" %zu", offsetof(skh_instance_motion, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_rewind_info, {f}));\n' for f in info)
                   + 'printf(" %u %u\\n", SKH_MOTION_MOVED, SKH_MOTION_DROP); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0 and lib.skh_abi_version() == 5  # the ABI grew, it did not change
    assert out.stdout.split() == [b"96", b"32", b"0", b"48", b"84", b"88", b"0", b"8", b"16", b"24", b"1", b"2"]
    assert "skh_motion.h" in [os.path.basename(d) for d in build.DEPS]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_instance_motion_check
# ---------------------------------------------------------------------------------------------------------------------------------------------
def table(n=3, **edits):
    """n identity entries with flags MOVED; edits: name -> (entry, value) or (entry, index, value)"""
    t = np.zeros(n, S.INSTANCE_MOTION)
    t["to_prev"], t["normal_to_prev"], t["flags"] = IDENTITY, np.eye(3, dtype=f32).reshape(9), S.MOTION_MOVED
    for name, e in edits.items():
        if len(e) == 2:
            t[name][e[0]] = e[1]
        else:
            t[name][e[0]][e[1]] = e[2]
    return t


ACCEPTED = {"moved entries": table(), "one entry": table(1), "an unmoved entry": table(flags=(1, 0)), "a dropped entry": table(flags=(2, 3)),
            "nan in an unmoved entry": table(flags=(0, 0), to_prev=(0, 3, np.nan)), "inf in a dropped entry": table(flags=(1, 3), normal_to_prev=(1, 8, np.inf)),
            "a huge entry": table(to_prev=(2, 11, 3e38)), "an empty table": table(0)}
REFUSED = {"flag bit 2": table(flags=(0, 5)), "flag bit 31": table(flags=(2, 0x80000001)), "DROP without MOVED": table(flags=(1, 2)), "reserved[0]": table(reserved=(0, 0, 1)),
           "reserved[1]": table(reserved=(2, 1, 7)), "nan position word": table(to_prev=(1, 0, np.nan)), "inf translation": table(to_prev=(2, 11, np.inf)),
           "-inf normal word": table(normal_to_prev=(0, 4, -np.inf)), "nan normal word in the last entry": table(5, normal_to_prev=(4, 8, np.nan))}


def test_motion_check_accepts_and_refuses(lib):
    for name, t in ACCEPTED.items():
        assert capi.instance_motion_check(t), name
    for name, t in REFUSED.items():
        assert not capi.instance_motion_check(t), name
        assert lib.skh_instance_motion_check(t.ctypes.data_as(C.c_void_p), len(t)) == 3, name
    assert lib.skh_instance_motion_check(None, 1) == 3 and lib.skh_instance_motion_check(None, 0) == 0
    # without a context (or without pointers) the entry points refuse instead of crashing
    assert lib.skh_set_instance_motion(None, None, 0) == 3 and lib.skh_rewind_guides(None, 1, 1, None, None, None, None, None) == 3
    assert lib.skh_get_rewind_info(None, None) == 3 and lib.skh_instance_motion_from_transforms(None, None, None) == 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_instance_motion_from_transforms
# ---------------------------------------------------------------------------------------------------------------------------------------------
def random_linear(rs):
    """rotation . diag(s) . rotation with s in [0.3, 3]: any 3 x 3 of condition number <= 10 has this form (its singular value decomposition)"""
    s = rs.uniform(0.3, 3.0, 3)
    L = M._rotation(rs.normal(size=3), rs.uniform(-180, 180)) @ np.diag(s) @ M._rotation(rs.normal(size=3), rs.uniform(-180, 180))
    return L * (1.0 if rs.uniform() < 0.8 else -1.0)  # (one in five mirrored)


def test_the_helper_against_numpy_on_random_transform_pairs(lib):
    """The helper works in double and rounds each entry once: 2^-24 |entry| from the rounding, and double's own error, cond x 2^-53 relative to the largest entry,
    is far below that.  The bar 2^-23 max|entry| cond, cond the larger condition number of the two float32 linear parts, holds both with room."""
    rs = np.random.RandomState(3)
    worst = 0.0
    for _ in range(200):
        a, b = transform(random_linear(rs), rs.uniform(-5, 5, 3)), transform(random_linear(rs), rs.uniform(-5, 5, 3))
        cond = max(np.linalg.cond(x.astype(np.float64).reshape(3, 4)[:, :3]) for x in (a, b))
        assert cond <= 10.0
        e = derive(a, b)
        want_p, want_n = M.motion64(a, b)
        assert int(e["flags"]) == S.MOTION_MOVED and not e["reserved"].any()
        for got, want in ((e["to_prev"].reshape(3, 4), want_p), (e["normal_to_prev"].reshape(3, 3), want_n)):
            bar = 2.0 ** -23 * np.abs(want).max() * cond
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / bar))
    print(f"skh_instance_motion_from_transforms against numpy on 200 pairs: worst error / (2^-23 max|entry| cond) {worst:.3f}")
    assert worst <= 1.0
    assert capi.instance_motion_check(np.array([derive(a, b)]))


def test_the_helper_equal_singular_nan_and_mirrored(lib):
    rs = np.random.RandomState(4)
    a = transform(random_linear(rs), (1, 2, 3))
    same = derive(a, a.copy())
    assert int(same["flags"]) == 0 and np.array_equal(same["to_prev"], IDENTITY) and np.array_equal(same["normal_to_prev"], np.eye(3, dtype=f32).reshape(9))
    flat = transform(np.diag([1.0, 0.0, 1.0]))
    nan = a.copy()
    nan[5] = np.nan
    inf = a.copy()
    inf[11] = np.inf
    for prev, cur in ((a, flat), (flat, a), (a, nan), (nan, a), (inf, a), (transform(np.eye(3) * 1e-30), transform(np.eye(3) * 1e30))):
        e = derive(prev, cur)
        assert int(e["flags"]) == S.MOTION_MOVED | S.MOTION_DROP and np.isfinite(e["to_prev"]).all() and np.isfinite(e["normal_to_prev"]).all()
        assert capi.instance_motion_check(np.array([e]))
    # -0 and +0 are different words: not "equal", and the entry that comes out is the identity map, MOVED
    z = a.copy()
    z[3] = 0.0
    nz = z.copy()
    nz[3] = -0.0
    assert int(derive(z, nz)["flags"]) == S.MOTION_MOVED
    # a mirror between the frames: the normal comes back with its own sign (the inverse transpose, not the cofactor matrix)
    A = M._rotation((1, 2, 3), 40.0) @ np.diag([1.2, 0.7, 1.0])
    B = np.diag([-1.0, 1.0, 1.0]) @ A
    e = derive(transform(A, (0.5, 0, 0)), transform(B, (0, 1, 0)))
    K = e["normal_to_prev"].astype(np.float64).reshape(3, 3)
    assert np.linalg.det(K) < 0
    for n_obj in np.eye(3):
        n_prev, n_cur = np.linalg.inv(A).T @ n_obj, np.linalg.inv(B).T @ n_obj
        back = K @ (n_cur / np.linalg.norm(n_cur))
        assert np.dot(back, n_prev) / (np.linalg.norm(back) * np.linalg.norm(n_prev)) > 1 - 1e-6


def bits_of(t):
    return np.ascontiguousarray(t).view(np.uint32).reshape(len(t), 24)


def test_scene_instance_motion_is_the_helper_entry_by_entry(lib):
    rs = np.random.RandomState(6)
    prev, cur = np.zeros(4, S.INSTANCE), np.zeros(5, S.INSTANCE)
    for i in range(4):
        prev["transform"][i] = transform(random_linear(rs), rs.uniform(-2, 2, 3))
    cur["transform"][:4] = prev["transform"]
    cur["transform"][1] = transform(random_linear(rs), rs.uniform(-2, 2, 3))
    cur["transform"][4] = prev["transform"][0]
    t = S.instance_motion(prev, cur)
    assert t.dtype == S.INSTANCE_MOTION and list(t["flags"]) == [0, 1, 0, 0, 3]  # (the instance the previous table lacks has no history)
    assert np.array_equal(bits_of(t)[1], bits_of(np.array([derive(prev["transform"][1], cur["transform"][1])]))[0])
    assert capi.instance_motion_check(t)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the definition: float32 inside float64's bar, and closed forms
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_input_meets_its_conditions(syn):
    ids = syn["ids"]
    kind, inst = ids[..., 3], ids[..., 0]
    surface = (kind == 1) | (kind == 2)
    assert ids.shape == (45, 67, 4) and len(syn["table"]) == M.N_INSTANCES
    assert list(syn["table"]["flags"]) == [0, 3, 1, 1, 1]  # the floor unmoved, the wall dropped, the box, the sphere and an entry nobody has moved
    assert (kind == 0).sum() >= 24 and (inst[kind == 0] == 0xFFFFFFFF).all() and (kind == 3).sum() >= 12
    assert (surface & (inst >= M.N_INSTANCES)).sum() == 6  # (surface pixels of an instance past the table's end)
    for i in range(4):
        assert (surface & (inst == i)).sum() >= 100, i
    for name in ("box", "sphere"):  # a rotation, a non-uniform scale in [0.6, 1.4], a translation
        X, _ = M.motion64(M.POSES_NOW[name], M.POSES_PREV[name])  # (previous -> current)
        sv = np.linalg.svd(X[:, :3], compute_uv=False)
        assert 0.6 <= sv.min() < sv.max() <= 1.4 and sv.max() / sv.min() > 1.2 and np.linalg.norm(X[:, 3]) > 0.2
        assert np.abs(X[:, :3] / np.linalg.norm(X[:, :3], axis=0) - np.eye(3)).max() > 0.1  # (its columns turned)
    assert not np.array_equal(np.asarray(syn["matrix"]), T.world_to_clip(T.camera((0.35, 1.35, 1.9), (-0.1, 0.55, -2.0), 55.0, 67 / 45.0)))  # (the camera moved too)
    # the chained reference makes no decision inside its rounding error on more than 1 % of the surface pixels
    r32 = M.rewind32(ids, syn["position"], syn["normal"], syn["table"])
    ref = T.reproject64(syn["color"], ids, r32["normal"], r32["position"], syn["albedo"], syn["prev"], syn["params"])
    share = ref["ambiguous"].sum() / ref["surface"].sum()
    print(f"synthetic 67 x 45 with moved instances: {int(ref['surface'].sum())} surface pixels, {int(syn['moved'].sum())} on moved instances; ambiguous after the "
          f"rewind {int(ref['ambiguous'].sum())} ({100 * share:.3f} %)")
    assert share <= 0.01


def test_float32_evaluation_stays_inside_the_bar(syn):
    for n in (1, M.N_INSTANCES):
        t = syn["table"][:n].copy()
        if n == 1:
            t[0] = syn["table"][2]  # (one entry, a moved one: the floor takes the box's motion, everything else is past the end)
        got, ref = M.rewind32(syn["ids"], syn["position"], syn["normal"], t), M.rewind64(syn["ids"], syn["position"], syn["normal"], t)
        ratio = M.check(got, ref)
        moved = ref["applies"] & ~ref["drop"]
        print(f"rewind32 against rewind64, n = {n}: {int(moved.sum())} moved, {int(ref['drop'].sum())} dropped pixels; worst error / bar {ratio:.3f}; "
              f"largest bar: position {ref['bar_position'].max():.2e}, normal {ref['bar_normal'].max():.2e}")
        assert moved.sum() > 300 and 0.005 < ratio <= 1.0
        assert ref["bar_position"].max() < 1e-5 and ref["bar_normal"].max() < 1e-5  # (the bar is a rounding bar, not a tolerance)
        # a different definition falls outside it: the normal through to_prev's linear part instead of its inverse transpose
        wrong = t.copy()
        wrong["normal_to_prev"] = t["to_prev"].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9)
        bad = M.rewind32(syn["ids"], syn["position"], syn["normal"], wrong)
        assert M.check({"position": got["position"], "normal": bad["normal"]}, ref) > 100.0


def plane(h, w, xyz, wword=1.0):
    a = np.zeros((h, w, 4), f32)
    a[..., :3], a[..., 3] = xyz, wword
    return a


def ids_plane(h, w, inst, kind):
    a = np.zeros((h, w, 4), np.uint32)
    a[..., 0], a[..., 2], a[..., 3] = inst, inst, kind
    return a


def test_closed_forms_bit_for_bit(lib):
    rs = np.random.RandomState(8)
    h, w = 6, 9
    P, N = plane(h, w, rs.uniform(-3, 3, (h, w, 3))), plane(h, w, rs.normal(size=(h, w, 3)))
    P.view(np.uint32)[0, 0, :] = [0x7FC01234, 0xFFC00001, 0x7F800000, 0x7FBFFFFF]  # (payloads a copy must keep)
    N.view(np.uint32)[0, 1, :] = [0xFFFFFFFF, 0x80000000, 0x00000001, 0xDEADBEEF]
    moved = derive(IDENTITY, transform(M._rotation((1, 1, 0), 33.0) @ np.diag([0.7, 1.3, 1.0]), (0.3, -0.2, 0.9)))
    t = np.array([derive(IDENTITY, IDENTITY), moved, moved])
    t[2]["flags"] = S.MOTION_MOVED | S.MOTION_DROP
    # copied: an unmoved entry, an instance past the end, 0xffffffff, and what is no surface pixel (a miss, a light proxy, kinds that do not exist)
    for inst, kind in ((0, 1), (0, 2), (3, 1), (0xFFFFFFFF, 1), (1, 0), (1, 3), (1, 4), (1, 0xFFFFFFFF), (2, 3)):
        out = M.rewind32(ids_plane(h, w, inst, kind), P, N, t)
        assert np.array_equal(M.bits(out["position"]), M.bits(P)) and np.array_equal(M.bits(out["normal"]), M.bits(N)), (inst, kind)
    # ... and a moved one is not
    out = M.rewind32(ids_plane(h, w, 1, 2), P, N, t)
    assert (M.bits(out["position"])[1:, :, :3] != M.bits(P)[1:, :, :3]).all() and np.array_equal(M.bits(out["position"])[..., 3], M.bits(P)[..., 3])
    assert np.array_equal(M.bits(out["normal"])[..., 3], M.bits(N)[..., 3])
    assert np.abs(np.linalg.norm(out["normal"][1:, :, :3].astype(np.float64), axis=-1) - 1).max() < 1e-6
    # DROP: the quiet NaN in the three position words, the normal copied
    out = M.rewind32(ids_plane(h, w, 2, 1), P, N, t)
    assert (M.bits(out["position"])[..., :3] == 0x7FC00000).all() and np.array_equal(M.bits(out["position"])[..., 3], M.bits(P)[..., 3])
    assert np.array_equal(M.bits(out["normal"]), M.bits(N))
    # a translation by exactly representable amounts: P + t' exactly (t' = -t, the way back), the axis normals unchanged
    Pq = plane(h, w, np.round(rs.uniform(-3, 3, (h, w, 3)) * 64) / 64)
    Nq = plane(h, w, np.eye(3)[rs.randint(0, 3, (h, w))] * rs.choice([-1.0, 1.0], (h, w, 1)))
    shift = np.array([0.5, -0.25, 2.0])
    e = derive(transform(np.eye(3), (1.0, 1.0, 1.0)), transform(np.eye(3), np.array([1.0, 1.0, 1.0]) + shift))
    assert int(e["flags"]) == 1 and np.array_equal(e["to_prev"].reshape(3, 4)[:, 3], (-shift).astype(f32))
    out = M.rewind32(ids_plane(h, w, 0, 1), Pq, Nq, np.array([e]))
    assert np.array_equal(out["position"][..., :3], (Pq[..., :3].astype(np.float64) - shift).astype(f32))
    assert np.array_equal(out["normal"][..., :3], Nq[..., :3]) and np.array_equal(M.bits(out["normal"])[..., 3], M.bits(Nq)[..., 3])
    # a quarter turn about z since the previous frame: going back permutes the components, (x, y, z) -> (y, -x, z)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    e = derive(IDENTITY, transform(Rz))
    Pn = plane(h, w, rs.uniform(0.5, 3, (h, w, 3)))  # (no zero component: the sign of a zero is not the subject)
    Nn = plane(h, w, np.array([0.6, 0.8, 0.0]))
    out = M.rewind32(ids_plane(h, w, 0, 1), Pn, Nn, np.array([e]))
    assert np.array_equal(out["position"][..., 0], Pn[..., 1]) and np.array_equal(out["position"][..., 1], -Pn[..., 0]) and np.array_equal(out["position"][..., 2], Pn[..., 2])
    v = np.array([0.8, -0.6, 0.0], f32)
    s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    assert np.array_equal(out["normal"][0, 0, :3], v / np.sqrt(s))  # (the permuted normal, renormalised by the definition's own operations)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the chain: what the rewound planes do to skh_temporal's definition
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_rewound_planes_find_the_history_that_the_true_planes_reject(syn):
    ids, p = syn["ids"], syn["params"]
    r32 = M.rewind32(ids, syn["position"], syn["normal"], syn["table"])
    rewound = T.reproject32(syn["color"], ids, r32["normal"], r32["position"], syn["albedo"], syn["prev"], p)
    true = T.reproject32(syn["color"], ids, syn["normal"], syn["position"], syn["albedo"], syn["prev"], p)
    ref = T.reproject64(syn["color"], ids, r32["normal"], r32["position"], syn["albedo"], syn["prev"], p)
    on = syn["moved"] & ref["projects"]
    mask, mask_true = rewound["motion"][..., 3], true["motion"][..., 3]
    four = float((mask[on] == 15).mean())
    # the previous surface at the rewound point is the plane through P* with the normal N*; the current point lies |N* . (P* - P)| off it.  The plane test sees
    # d = N . (P'(q) - P) with P'(q) where the previous camera's ray through P met that plane: the same distance up to the ratio of two cosines that the
    # normal test keeps near 1.  Twice the tolerance leaves that ratio, and the taps' one-pixel offsets, their room.
    off = np.abs(((r32["position"][..., :3].astype(np.float64) - syn["position"][..., :3]) * r32["normal"][..., :3]).sum(-1))
    far = on & (off > 2 * float(p["plane_tolerance"]))
    print(f"synthetic 67 x 45: {int(on.sum())} pixels of the moved instances project; all four taps accepted on the rewound planes {four:.3f}; {int(far.sum())} lie more "
          f"than twice the tolerance off the previous surface, of which the true planes accept a tap on {int((mask_true[far] != 0).sum())}")
    assert on.sum() > 300 and four > 0.5
    assert far.sum() > 0.8 * on.sum() and (mask_true[far] == 0).all()
    # the wall's pixels were dropped: they do not project; the floor (unmoved) is what it is without the rewind
    wall = (ids[..., 0] == 1) & (ids[..., 3] == 1)
    assert not rewound["motion"][wall].any() and (rewound["history"][wall][:, 3] == 1.0).all() and true["motion"][wall].any()
    floor = (ids[..., 0] == 0) & (ids[..., 3] == 1)
    for n in ("image", "history", "motion"):
        assert np.array_equal(M.bits(rewound[n])[floor], M.bits(true[n])[floor]), n
