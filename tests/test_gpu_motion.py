"""Object motion on the device (skh_set_instance_motion, skh_rewind_guides; DESIGN.md section 2, "Object motion").  The definition has no transcendental, so the
device must give the bits of its float32 restatement (tests/motionref.py: rewind32) on every word of both planes; the float64 reference with its written-out
error bar (rewind64) is the second, independent yardstick, and no pixel is excluded from it.  Chained with skh_temporal and skh_moments the rewound planes must give
the bits of the chained restatements, and on rendered scenes with moved instances the history must survive where, without the rewind, the plane test rejects it.
Every test calls the new entry points, so each fails without the feature.

Figures on an MI355X: docs/LOG.md has the lines the tests print."""

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import motionref as M
from tests import temporalref as T
from tests import varianceref as V

pytestmark = pytest.mark.gpu

OUTPUTS = ("image", "history", "motion")
bits = M.bits


@pytest.fixture(scope="module")
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def syn():
    return M.synthetic()


class Planes:
    """device copies of an IDS, a POSITION and a NORMAL plane, and two output planes"""

    def __init__(self, ctx, ids, position, normal):
        self.ctx, self.h, self.w = ctx, ids.shape[0], ids.shape[1]
        self.host = {"ids": np.ascontiguousarray(ids, np.uint32), "position": np.ascontiguousarray(position, np.float32), "normal": np.ascontiguousarray(normal, np.float32)}
        self.d = {n: ctx.buffer_alloc(16 * self.w * self.h) for n in ("ids", "position", "normal", "position_out", "normal_out")}
        for n, a in self.host.items():
            ctx.buffer_upload(self.d[n], a)

    def fill(self, name, value):
        self.ctx.buffer_upload(self.d[name], np.full((self.h, self.w, 4), value, np.float32))

    def download(self, name):
        out = np.zeros((self.h, self.w, 4), np.float32)
        self.ctx.buffer_download(self.d[name], out)
        return out

    def rewind(self, po="position_out", no="normal_out", width=None, height=None, **null):
        """the call, writing into the planes named `po` and `no`; `null`: planes handed over as NULL"""
        d = dict(self.d)
        d.update(null)
        self.ctx.rewind_guides_device(self.w if width is None else width, self.h if height is None else height, d["ids"], d["position"], d["normal"], d[po], d[no])
        return {"position": self.download(po), "normal": self.download(no)}

    def free(self):
        for v in self.d.values():
            self.ctx.buffer_free(v)


def random_input(w, h, n, seed):
    """random planes that take every branch at any size: instance ids below, at and past the table's end and 0xffffffff, kinds 0 .. 3, positions and normals with
    NaN, infinity and zero among them; a table of n entries of mixed flags whose first entry is moved"""
    rs = np.random.RandomState(seed)
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 0] = rs.choice(list(range(n + 2)) + [0xFFFFFFFF, 0x80000000], size=(h, w))
    ids[..., 1], ids[..., 2] = rs.randint(0, 1000, (h, w)), ids[..., 0]
    ids[..., 3] = rs.choice([0, 1, 1, 1, 2, 2, 3, 7], size=(h, w))
    P, N = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    P[..., :3], N[..., :3] = rs.uniform(-4, 4, (h, w, 3)), rs.normal(size=(h, w, 3))
    N[..., :3] /= np.linalg.norm(N[..., :3], axis=-1, keepdims=True)
    P[..., 3], N[..., 3] = rs.uniform(0, 1, (h, w)), rs.uniform(0, 1, (h, w))
    odd = rs.uniform(size=(h, w))
    P[odd < 0.03, 0], P[(odd > 0.03) & (odd < 0.05), 2], N[(odd > 0.05) & (odd < 0.08), 1], N[(odd > 0.08) & (odd < 0.1), :3] = np.nan, np.inf, np.nan, 0.0
    P.view(np.uint32)[0, 0, 3], N.view(np.uint32)[0, 0, 3] = 0x7FC01234, 0xFFFFFFFF
    prev = [M.pose(rs.uniform(-1, 1, 3), rs.normal(size=3), rs.uniform(-90, 90), rs.uniform(0.6, 1.4, 3)) for _ in range(n)]
    cur = [M.pose(rs.uniform(-1, 1, 3), rs.normal(size=3), rs.uniform(-90, 90), rs.uniform(0.6, 1.4, 3)) for _ in range(n)]
    table = M.table_from(prev, cur)
    for i in range(1, n):
        table[i]["flags"] = (M.MOVED, 0, M.MOVED | M.DROP, M.MOVED)[i % 4]
    return ids, P, N, table


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the bits, and the bar; 2. in place
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("w,h", [(67, 45), (1, 1), (1, 300), (300, 1), (64, 64), (65, 63)])
def test_bit_for_bit_and_inside_the_bar_in_place_too(ctx, syn, w, h, n):
    if (w, h) == (67, 45):
        ids, P, N, table = syn["ids"], syn["position"], syn["normal"], syn["table"][:n].copy()
        if n == 1:
            table[0] = syn["table"][2]
    else:
        ids, P, N, table = random_input(w, h, n, 100 * w + h + n)
    pl = Planes(ctx, ids, P, N)
    try:
        ctx.set_instance_motion(table)
        assert ctx.rewind_info()["entries"] == n
        got = pl.rewind()
        want, ref = M.rewind32(ids, P, N, table), M.rewind64(ids, P, N, table)
        differing = {k: int((bits(got[k]) != bits(want[k])).any(axis=-1).sum()) for k in ("position", "normal")}
        ratio = M.check(got, ref)
        print(f"{w} x {h}, n = {n}: pixels that differ from the float32 restatement {differing} of {w * h}; {int((ref['applies'] & ~ref['drop']).sum())} moved, "
              f"{int(ref['drop'].sum())} dropped; worst error / float64 bar {ratio:.3f}")
        for k in ("position", "normal"):
            assert M.same_words(got[k], want[k]), k
        assert ratio <= 1.0  # (check() has compared every copied and constant word as bits)
        # the inputs were not written
        assert np.array_equal(bits(pl.download("position")), bits(P)) and np.array_equal(bits(pl.download("normal")), bits(N))
        # in place: one plane, then the other, then both
        for po, no in (("position", "normal_out"), ("position_out", "normal"), ("position", "normal")):
            for k in ("position", "normal"):
                ctx.buffer_upload(pl.d[k], pl.host[k])
            again = pl.rewind(po, no)
            for k in ("position", "normal"):
                assert np.array_equal(bits(again[k]), bits(got[k])), (po, no, k)
    finally:
        pl.free()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. refusals and the table's life
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_table_lives_as_documented(syn):
    from strelka_amd import capi

    c = capi.Context(0)
    pl = Planes(c, syn["ids"], syn["position"], syn["normal"])
    outs = ("position_out", "normal_out")

    def untouched():
        return all((pl.download(k) == 7.25).all() for k in outs)

    try:
        for k in outs:
            pl.fill(k, 7.25)
        assert c.rewind_info() == {"calls": 0, "pixels": 0, "ms_last": 0.0, "entries": 0}
        with pytest.raises(capi.SkhError, match="skh_rewind_guides"):  # no table yet
            pl.rewind()
        assert untouched()
        small = syn["table"][:1].copy()
        small[0] = syn["table"][2]
        c.set_instance_motion(small)
        assert c.rewind_info()["entries"] == 1
        first = pl.rewind()
        assert np.array_equal(bits(first["position"]), bits(M.rewind32(syn["ids"], syn["position"], syn["normal"], small)["position"]))
        c.set_instance_motion(syn["table"])  # replaced by a larger one
        assert c.rewind_info()["entries"] == M.N_INSTANCES
        want = M.rewind32(syn["ids"], syn["position"], syn["normal"], syn["table"])
        second = pl.rewind()
        assert all(np.array_equal(bits(second[k]), bits(want[k])) for k in want) and not np.array_equal(bits(second["position"]), bits(first["position"]))
        # refused tables leave the old one in force
        for k in outs:
            pl.fill(k, 7.25)
        bad = {}
        for name, edit in (("flag", ("flags", 4)), ("drop alone", ("flags", 2)), ("reserved", ("reserved", 1)), ("nan", ("to_prev", np.nan))):
            t = syn["table"].copy()
            t[edit[0]][2] = edit[1]
            bad[name] = t
        for name, t in bad.items():
            assert not capi.instance_motion_check(t), name
            with pytest.raises(capi.SkhError, match="skh_set_instance_motion"):
                c.set_instance_motion(t)
            assert c.rewind_info()["entries"] == M.N_INSTANCES, name
        assert c.lib.skh_set_instance_motion(c.h, None, 3) == 3 and c.rewind_info()["entries"] == M.N_INSTANCES
        # refused calls: nothing written, nothing counted
        before = c.rewind_info()
        cases = {"zero width": dict(width=0), "zero height": dict(height=0), "more than 2^26 pixels": dict(width=(1 << 13) + 1, height=1 << 13),
                 "a product that wraps 32 bits": dict(width=1 << 16, height=1 << 16)}
        cases.update({"no " + k: {k: None} for k in ("ids", "position", "normal", "position_out", "normal_out")})
        for name, kw in cases.items():
            with pytest.raises(capi.SkhError, match="skh_rewind_guides"):
                pl.rewind(**kw)
            assert untouched(), name
        after = c.rewind_info()
        assert (after["calls"], after["pixels"]) == (before["calls"], before["pixels"]) == (2, 2 * pl.w * pl.h) and before["ms_last"] > 0.0
        third = pl.rewind()  # (the table in force is still the larger one)
        assert all(np.array_equal(bits(third[k]), bits(want[k])) for k in want)
        # cleared: no table, the call is refused again; the counters are reset with the other statistics
        c.set_instance_motion(None)
        assert c.rewind_info()["entries"] == 0
        for k in outs:
            pl.fill(k, 7.25)
        with pytest.raises(capi.SkhError, match="skh_rewind_guides"):
            pl.rewind()
        assert untouched() and c.rewind_info()["calls"] == 3
        c.reset_stats()
        info = c.rewind_info()
        assert (info["calls"], info["pixels"], info["entries"]) == (0, 0, 0)
        c.set_instance_motion(small)  # (and set again after a clear)
        assert np.array_equal(bits(pl.rewind()["position"]), bits(first["position"])) and c.rewind_info()["calls"] == 1
    finally:
        pl.free()
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. - 6. rendered scenes
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


def block_face_normals(instances, index):
    """the five faces of a block of cornell_blocks() in world space"""
    L = np.asarray(instances["transform"][index], np.float64).reshape(3, 4)[:, :3]
    return [L @ np.array(a, np.float64) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1))]


def project64(matrix, P, W, H):
    clip = np.concatenate([P, np.ones(P.shape[:-1] + (1,))], -1) @ np.asarray(matrix, np.float64).reshape(4, 4).T
    with np.errstate(all="ignore"):
        return (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W - 0.5, (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H - 0.5, clip[..., 3]


def chain(c, raw, guides, prev, p, table):
    """device rewind then device skh_temporal, against rewind32 then reproject32: bit for bit on both planes and all three outputs"""
    c.set_instance_motion(table)
    rw = c.rewind_guides(guides)
    want_rw = M.rewind32(guides["ids"], guides["position"], guides["normal"], table)
    for k in ("position", "normal"):
        assert np.array_equal(bits(rw[k]), bits(want_rw[k])), k
    rewound = dict(guides, position=rw["position"], normal=rw["normal"])
    got = c.temporal(raw, rewound, prev, p)
    want = T.reproject32(raw, guides["ids"], want_rw["normal"], want_rw["position"], guides["albedo"], prev, p)
    for n in OUTPUTS:
        assert np.array_equal(bits(got[n]), bits(want[n])), n
    return rw, got


def test_cornell_blocks_a_translated_block_keeps_its_history_and_the_frame_is_untouched():
    from strelka_amd import capi

    W, H = 96, 64
    SHORT = scenes.CORNELL_BLOCKS_SHORT
    t = np.array([0.12, 0.08, 0.10])
    sc = scenes.cornell_blocks()
    arr = sc.arrays()
    assert len(arr["instances"]) == 6
    cam = sc.getCamera()
    moved_instances = translated(arr["instances"], SHORT, t)
    p0 = S.temporal_params(W, H, scene=arr)
    tol = float(p0["plane_tolerance"])
    for nf in block_face_normals(arr["instances"], SHORT):  # the precondition: without the rewind the plane test must reject every tap on the block
        assert abs(np.dot(nf, t)) >= 3 * tol, (nf, tol)
    a, b = capi.Context(0), capi.Context(0)
    try:
        for c in (a, b):
            c.set_scene(arr)
            c.resize(W, H)
        d_image = a.buffer_alloc(16 * W * H)
        aov = S.aov_params(cam, W, H)
        guides0 = a.render_guides(aov)
        raw0 = sample_frame(a, cam, W, H, 0, d_image)
        for c in (a, b):
            c.update_accel(moved_instances)
        guides1 = a.render_guides(aov)
        raw1 = sample_frame(a, cam, W, H, 1, d_image)
        # an accumulation in progress, beside a context that never hears of the feature
        for c in (a, b):
            for i in range(3):
                c.render_subframe(S.frame_params(cam, W, H, subframe_index=i, spp_total=64, max_depth=4))
        accum, stats, adaptive = a.read_accum(), a.stats(), a.adaptive_info()
        first = a.temporal(raw0, guides0, None, p0)
        p1 = S.temporal_params(W, H, aov, scene=arr)
        prev = {"history": first["history"], "ids": guides0["ids"], "normal": guides0["normal"], "position": guides0["position"]}
        table = S.instance_motion(arr["instances"], moved_instances)
        assert list(table["flags"]) == [0, 0, 0, 1, 0, 0]
        rw, got = chain(a, raw1, guides1, prev, p1, table)
        without = a.temporal(raw1, guides1, prev, p1)
        # the frame did not move
        after = a.stats()
        assert np.array_equal(bits(a.read_accum()), bits(accum)) and a.adaptive_info() == adaptive
        assert all(after[k] == stats[k] for k in after if k.startswith("rays_")) and after["speculated_discarded"] == stats["speculated_discarded"]
        for c in (a, b):
            c.render_subframe(S.frame_params(cam, W, H, subframe_index=3, spp_total=64, max_depth=4))
        assert np.array_equal(bits(a.read_accum()), bits(b.read_accum()))
        info = a.rewind_info()
        assert (info["calls"], info["pixels"], info["entries"]) == (1, W * H, 6) and info["ms_last"] > 0.0 and b.rewind_info()["calls"] == 0
        # the block's pixels
        ids1, ids0 = guides1["ids"], guides0["ids"]
        block = (ids1[..., 0] == SHORT) & (ids1[..., 3] == 1) & np.isfinite(raw1[..., :3]).all(-1)
        assert block.sum() > 150
        to_prev, _ = M.motion64(arr["instances"]["transform"][SHORT], moved_instances["transform"][SHORT])
        P = guides1["position"][..., :3].astype(np.float64)
        Pprev = P @ to_prev[:, :3].T + to_prev[:, 3]
        assert np.abs(Pprev - (P - t))[block].max() < 1e-6
        fx, fy, cw = project64(aov["world_to_clip"], Pprev, W, H)
        yy, xx = np.mgrid[0:H, 0:W]
        inside = block & (cw > 0) & (fx > -0.99) & (fx < W - 0.01) & (fy > -0.99) & (fy < H - 0.01)
        mv = got["motion"].astype(np.float64)
        assert inside.sum() > 0.9 * block.sum()
        assert np.abs(mv[..., 0] - (fx - xx))[inside].max() < 1e-3 and np.abs(mv[..., 1] - (fy - yy))[inside].max() < 1e-3
        assert np.hypot(mv[..., 0], mv[..., 1])[inside].min() > 1.0  # (the block moved by several pixels)
        # every other pixel: what skh_temporal gives without the rewind, bit for bit -- all three outputs
        for n in OUTPUTS:
            assert np.array_equal(bits(got[n])[~block], bits(without[n])[~block]), n
        # history: kept with the rewind where all four taps saw the block a frame ago, lost without it on every pixel of the block
        ix, iy = np.floor(np.where(inside, mv[..., 0] + xx, 0)).astype(int), np.floor(np.where(inside, mv[..., 1] + yy, 0)).astype(int)
        on_block = inside.copy()
        for dx, dy in T.TAPS:
            qx, qy = ix + dx, iy + dy
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            on_block &= ok & (ids0[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1), 0] == SHORT) & (ids0[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1), 3] == 1)
        kept = float((got["history"][..., 3][on_block] > 1.0).mean())
        print(f"cornell blocks {W} x {H}, the short block translated by {tuple(t.tolist())}: {int(block.sum())} pixels on it, {int(on_block.sum())} with all four taps on the block a frame "
              f"ago; history kept with the rewind on {kept:.3f} of those, four taps accepted on {float((got['motion'][..., 3][on_block] == 15).mean()):.3f}; without the rewind "
              f"accepted taps on {int((without['motion'][..., 3][block] != 0).sum())} of the block's pixels")
        assert on_block.sum() > 100 and kept > 0.7
        assert (without["motion"][..., 3][on_block] == 0).all() and (without["history"][..., 3][on_block] == 1.0).all()
        # 6. skh_moments on the rewound position with that call's motion plane: varianceref's bits
        m0 = a.moments(raw0, guides0, None, None, p0)
        rewound = dict(guides1, position=rw["position"], normal=rw["normal"])
        m1 = a.moments(raw1, rewound, got["motion"], m0, p1)
        want_m1 = V.moments32(raw1, ids1, rw["position"], guides1["albedo"], got["motion"], m0, p1)
        assert np.array_equal(bits(m1), bits(want_m1))
        m1_true = a.moments(raw1, guides1, without["motion"], m0, p1)
        assert (m1[..., 3][on_block] > 1.0).mean() > 0.7 and (m1_true[..., 3][on_block] == 1.0).all()  # (the moments' own history follows the block too)
        a.buffer_free(d_image)
    finally:
        a.close(), b.close()


def test_small_kitchen_a_third_of_the_instances_moved():
    from strelka_amd import capi
    from tests.test_gpu_parity import small_kitchen
    from tests.test_gpu_update import HALF_ROOM, _moved, _moves

    W, H = 96, 64
    sc = small_kitchen()
    arr = dict(sc.arrays())
    cam = sc.getCamera()
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    sel = mesh[::3]
    moved_instances = _moved(arr["instances"], sel, _moves(np.random.RandomState(21), len(sel), HALF_ROOM))
    # (a move is applied in world space, about the room's origin; carried back about the instance's own position so that the instance stays where the camera looks)
    for i in sel:
        a0, a1 = arr["instances"]["transform"][i].reshape(3, 4), moved_instances["transform"][i].reshape(3, 4)
        a1[:, 3] = a0[:, 3] + 0.1 * (a1[:, 3] - a0[:, 3])
    c = capi.Context(0)
    try:
        c.set_scene(arr)
        c.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        aov = S.aov_params(cam, W, H)
        guides0 = c.render_guides(aov)
        raw0 = sample_frame(c, cam, W, H, 0, d_image)
        c.update_accel(moved_instances)
        guides1 = c.render_guides(aov)
        raw1 = sample_frame(c, cam, W, H, 1, d_image)
        p0 = S.temporal_params(W, H, scene=arr)
        p1 = S.temporal_params(W, H, aov, scene=arr)
        first = c.temporal(raw0, guides0, None, p0)
        prev = {"history": first["history"], "ids": guides0["ids"], "normal": guides0["normal"], "position": guides0["position"]}
        table = S.instance_motion(arr["instances"], moved_instances)
        assert sorted(np.nonzero(table["flags"])[0]) == sorted(sel) and (table["flags"][sel] == 1).all()
        rw, got = chain(c, raw1, guides1, prev, p1, table)
        ids1 = guides1["ids"]
        kind = ids1[..., 3]
        on_moved = ((kind == 1) | (kind == 2)) & np.isin(ids1[..., 0], sel)
        ref = M.rewind64(ids1, guides1["position"], guides1["normal"], table)
        assert np.array_equal(ref["applies"], on_moved) and M.check(rw, ref) <= 1.0
        worst = 0.0
        for i in sel:
            px = on_moved & (ids1[..., 0] == i)
            if not px.any():
                continue
            X, _ = M.motion64(arr["instances"]["transform"][i], moved_instances["transform"][i])
            P = guides1["position"][..., :3].astype(np.float64)[px]
            want = P @ X[:, :3].T + X[:, 3]
            # rewind64's bar for the table's float32 words, and the words' own rounding: 2^-24 of each term of the row
            entry = table[i]["to_prev"].astype(np.float64).reshape(3, 4)
            slack = (np.abs(P) @ np.abs(X[:, :3] - entry[:, :3]).T + np.abs(X[:, 3] - entry[:, 3]))
            err = np.abs(rw["position"][..., :3].astype(np.float64)[px] - want)
            worst = max(worst, float((err / (ref["bar_position"][..., :3][px] + slack)).max()))
        surf = on_moved & np.isfinite(raw1[..., :3]).all(-1) & ((got["motion"][..., :3] != 0).any(-1))
        four = float((got["motion"][..., 3][surf] == 15).mean()) if surf.any() else float("nan")
        print(f"small kitchen {W} x {H}, {len(sel)} of {len(mesh)} mesh instances moved (rotation, non-uniform scale, translation): {int(on_moved.sum())} pixels on them, "
              f"{int(surf.sum())} project; rewound position against motion64 . P: worst error / bar {worst:.3f}; all four taps accepted on {four:.3f} of those that project")
        assert on_moved.sum() > 0 and worst <= 1.0
        c.buffer_free(d_image)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. a shaking block
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_shaking_block_is_closer_to_the_converged_frame_with_the_rewind():
    from strelka_amd import capi

    W = H = 128
    FRAMES = 12
    SHORT = scenes.CORNELL_BLOCKS_SHORT
    t = np.array([0.06, 0.04, 0.05])
    sc = scenes.cornell_blocks()
    arr = sc.arrays()
    cam = sc.getCamera()
    tol = float(S.temporal_params(W, H, scene=arr)["plane_tolerance"])
    for nf in block_face_normals(arr["instances"], SHORT):  # the block goes from -t to +t: twice |N . t| between two frames, and at least 1.5 tolerances each way
        assert abs(np.dot(nf, t)) >= 1.5 * tol, (nf, tol)
    poses = [translated(arr["instances"], SHORT, t if k % 2 == 0 else -t) for k in range(FRAMES)]
    c, truth = capi.Context(0), capi.Context(0)
    try:
        for x in (c, truth):
            x.set_scene(arr)
            x.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        aov = S.aov_params(cam, W, H)
        prev = {True: None, False: None}
        out = {}
        for k in range(FRAMES):
            c.update_accel(poses[k])
            guides = c.render_guides(aov)
            raw = sample_frame(c, cam, W, H, k, d_image)
            p = S.temporal_params(W, H, aov if k else None, scene=arr)
            for rewind in (True, False):
                g = guides
                if rewind and k:
                    c.set_instance_motion(S.instance_motion(poses[k - 1], poses[k]))
                    rw = c.rewind_guides(guides)
                    g = dict(guides, position=rw["position"], normal=rw["normal"])
                out[rewind] = c.temporal(raw, g, prev[rewind], p)
                prev[rewind] = {"history": out[rewind]["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}
        c.buffer_free(d_image)
        truth.update_accel(poses[-1])
        truth.render_subframes(S.frame_params(cam, W, H, subframe_index=0, spp_total=1024, max_depth=4), 1024)
        want = truth.read_accum()[..., :3].astype(np.float64)
        block = (guides["ids"][..., 0] == SHORT) & (guides["ids"][..., 3] == 1) & np.isfinite(raw[..., :3]).all(-1)
        rms = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - want)[block] ** 2).mean()))
        e_raw, e_with, e_without = rms(raw), rms(out[True]["image"]), rms(out[False]["image"])
        n_with, n_without = out[True]["history"][..., 3][block], out[False]["history"][..., 3][block]
        print(f"cornell blocks {W} x {H}, the short block shaking by +-{tuple(t.tolist())}, frame {FRAMES} at one sample per frame; rms error against 1024 spp over the block's "
              f"{int(block.sum())} pixels: raw {e_raw:.5f}, temporal without the rewind {e_without:.5f}, with it {e_with:.5f} (ratio {e_with / e_without:.3f}); history length on "
              f"the block: mean {n_with.mean():.2f} with, {n_without.mean():.2f} without")
        assert block.sum() > 300 and e_with < e_without
    finally:
        c.close(), truth.close()
