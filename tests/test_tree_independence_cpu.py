"""tests/treeref.py held to itself and the checker held to it, on the CPU: the scenes are what their docstrings say, enough of their rays are decided and hit (from
treeref alone, before any renderer is looked at), the checker's hierarchy equals its brute-force loop bit for bit on every scene -- closest hit and any-hit -- and on
the decided rays the checker names the float64 primitive with t, u, v inside the bars.  tests/test_gpu_tree_independence.py asks the same of the device's trees."""
import numpy as np
import pytest

from tests import treeref as R

NAMES = sorted(R.SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_enough_rays_are_decided_and_hit(name):
    scene, arr, (inst, prim, W), rays, ref, shadow = R.cached(name)
    undecided, hit = R.shares(name)
    print("%s: %d triangles, %d rays, %d any-hit twins, undecided %.4f, decided hits %.4f" % (name, len(W), len(rays), len(shadow), undecided, hit))
    assert len(W) <= 4000 and len(rays) <= 20000 and len(shadow) <= 20000
    assert undecided <= R.MAX_UNDECIDED, undecided
    assert hit >= R.MIN_HIT, hit
    assert len(np.unique(ref["family"])) >= 7  # every family of rays is there
    assert (rays["tmin"] == 0).all() and (rays["tmax"] == np.float32(1e16)).all() and (shadow["tmax"] < 1e3).all()


def _diagonal(quads, axis):
    """quads (n, 2, 3, 3): the sign of the slope, in the quad's plane, of the edge its two triangles share"""
    out = []
    for t0, t1 in quads:
        p, q = sorted(set(map(tuple, t0)) & set(map(tuple, t1)))
        out.append(np.sign((q[(axis + 1) % 3] - p[(axis + 1) % 3]) * (q[(axis + 2) % 3] - p[(axis + 2) % 3])))
    return np.array(out)


def test_the_scenes_are_what_they_claim():
    # flat_room: axis-aligned quads 2 ... 8 long, some on the coordinate planes; cabinets whose boxes nest
    W = R.cached("flat_room")[2][2]
    e = np.linalg.norm(W - np.roll(W, 1, axis=1), axis=2)
    n = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
    assert ((n != 0).sum(axis=1) == 1).all()  # every triangle lies in an axis-aligned plane
    room = W[:22]
    assert np.linalg.norm(room - np.roll(room, 1, axis=1), axis=2).max(axis=1).min() >= 2.0 and e.max() == 10.0
    assert sum(((np.abs(room[:, :, a]) == 0).all(axis=1)).any() for a in range(3)) == 3
    # coplanar_panels: every door lies in front of its front face by the stated offset, split along the other diagonal
    scene, arr, (inst, prim, W), rays, ref, shadow = R.cached("coplanar_panels")
    offs = set()
    for axis in range(3):
        m = W[inst == axis].reshape(-1, 14, 3, 3)
        front, door = m[:, 2 * (2 * axis + 1):2 * (2 * axis + 1) + 2], m[:, 12:14]
        assert (np.ptp(front[..., axis], axis=(1, 2)) == 0).all() and (np.ptp(door[..., axis], axis=(1, 2)) == 0).all()
        s = np.ptp(front[..., (axis + 1) % 3], axis=(1, 2))
        offs |= set(np.round((door[:, 0, 0, axis] - front[:, 0, 0, axis]) / s, 9))
        c = front[:, 0, 0, axis].astype(np.float32)
        assert (np.nextafter(c, np.float32(np.inf)).astype(np.float64) == door[:, 0, 0, axis]).sum() >= 1  # the one-ulp pair
        assert (_diagonal(front, axis) == -_diagonal(door, axis)).all()  # the two quads of a pair are split along different diagonals
    assert {0.0, 1e-6, 1e-5, 1e-4} <= offs, offs
    # slats and mechanism_scene: the stated aspects
    for name, lo, hi in (("slats", 50.0, 500.0), ("mechanism_scene", 1500.0, 1700.0)):
        scene, arr, (inst, prim, W), rays, ref, shadow = R.cached(name)
        k = (inst >= 1) & (inst <= len(scene.rods))
        e = np.linalg.norm(W[k] - np.roll(W[k], 1, axis=1), axis=2)
        aspect = e.max(axis=1) / e.min(axis=1)
        print(name, "aspects %.0f ... %.0f" % (aspect.min(), aspect.max()))
        assert aspect.min() >= 0.8 * lo and aspect.max() <= 1.25 * hi and aspect.max() >= 0.8 * hi
        axes = {int(np.argmax(np.abs(np.subtract(b, a)))) for a, b, r in scene.rods}
        assert axes == ({0, 1, 2} if name == "mechanism_scene" else {0, 2}), axes  # every branch of the dominant-axis select meets the slivers
    fam, aim, d = ref["family"], ref["aim"], np.asarray(rays["dir"], np.float64)  # mechanism_scene's silhouette rays: the rod's axis is the ray's dominant one, each axis in turn
    sil = fam == 6
    rod_axis = np.array([int(np.argmax(np.abs(np.subtract(b, a)))) for a, b, r in scene.rods])[inst[aim[sil]] - 1]
    assert (np.argmax(np.abs(d[sil]), axis=1) == rod_axis).all() and (np.bincount(rod_axis, minlength=3) >= 40).all(), np.bincount(rod_axis, minlength=3)


def test_the_ray_families_are_what_they_claim():
    scene, arr, (inst, prim, W), rays, ref, shadow = R.cached("flat_room")
    fam, d, o = ref["family"], np.asarray(rays["dir"], np.float64), np.asarray(rays["origin"], np.float64)
    axis = fam == 4
    assert ((d[axis] == 0).sum(axis=1) == 2).all() and np.signbit(d[axis]).any() and (~np.signbit(d[axis]) & (d[axis] == 0)).any()  # +0.0 and -0.0 both occur
    graz = np.nonzero(fam == 2)[0]
    k = ref["aim"][graz]  # the triangle each ray was aimed at: its plane is met at 1e-3 ... 1e-1 rad, <= 0.5 from the origin, the far vertex >= 10 times as far
    n = np.cross(W[k, 1] - W[k, 0], W[k, 2] - W[k, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ang = np.arcsin(np.abs((d[graz] * n).sum(1)))
    t_aim = ((W[k, 0] - o[graz]) * n).sum(1) / (d[graz] * n).sum(1)
    far = np.linalg.norm(W[k] - o[graz][:, None, :], axis=2).max(axis=1)
    assert (ang > 0.9e-3).all() and (ang < 0.11).all() and ang.min() < 2e-3 and ang.max() > 0.05
    # (the origin is rounded to float32, half an ulp per coordinate: across a plane met at `ang` that moves the crossing by up to 3 * 2^-24 |o| / sin(ang))
    tol = 3 * 2.0 ** -24 * (np.abs(o[graz]).max(axis=1) + 1.0) / np.sin(ang)
    assert (t_aim > 0.04).all() and (t_aim <= 0.5 + tol).all() and (far >= 10.0 * (t_aim - tol)).all() and (far >= 100.0 * t_aim).any()
    h = ref["hit"][graz]
    assert (ref["t"][graz][h] <= (t_aim + tol)[h]).all()  # (the hit is the aimed one or something nearer)
    edge = fam == 0
    assert not ref["decided"][edge].all()  # a ray through a shared edge has two answers
    tw = shadow["tmax"].astype(np.float64)
    assert len(shadow) and (tw > 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_checker_hierarchy_equals_its_brute_force_and_the_reference(name):
    from tests import orklib

    scene, arr, tri, rays, ref, shadow = R.cached(name)
    for bake in (4, 0):
        o = orklib.new_context()
        o.set_bake(bake)
        o.set_scene(arr)
        got, brute = o.trace(rays, 0), o.trace(rays, 0, brute=True)
        diff = np.nonzero(got != brute)[0]
        assert got.tobytes() == brute.tobytes(), "%s, bake %d: %d records depend on the checker's tree (first rays %s, families %s)" % (name, bake, len(diff), diff[:4], ref["family"][diff[:4]])
        assert np.array_equal(o.trace(shadow, 1)["t"].view(np.uint32), o.trace(shadow, 1, brute=True)["t"].view(np.uint32))
        assert o.trace(shadow, 0).tobytes() == o.trace(shadow, 0, brute=True).tobytes()
        wrong, ft, fb = R.check_decided(name, brute)
        print("%s, bake %d: t at %.3f of its bar, u / v at %.3f of theirs" % (name, bake, ft, fb))
        assert len(wrong) == 0, "%s: %d decided rays name another primitive than float64 (first %s)" % (name, len(wrong), wrong[:4])
        assert ft <= 1.0 and fb <= 1.0, (name, ft, fb)
