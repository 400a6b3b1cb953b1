"""Light shapes off the GPU ("Light shapes"): the ABI's three symbols and the record's layout; the header (csrc/skh_lshape.h through the
host compiler) against tests/lightref.py in float64; createLight's keys -> Scene.arrays()["light_shapes"]; the .skscene round trip; and the reference itself
against Lambert's polygon formula before anything is held to it."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S, scene_io, scenes
from tests import emitref, lightref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24  # half an ulp, relative


def test_symbols_are_declared_exported_and_bound(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "strelka_hip.h")).read()
    hip = open(os.path.join(ROOT, "strelka_amd", "csrc", "strelka_hip.hip")).read()
    for name in ("skh_set_light_shapes", "skh_get_light_shape_info", "skh_light_shape_probe"):
        assert re.search(r"skh_status %s\(skh_context\*" % name, hdr), name
        assert re.search(r"^skh_status %s\(skh_context\*" % name, hip, re.M), name  # defined inside the header's extern "C" declarations
        assert name in capi.SYMBOLS
    assert "#define SKH_ABI_VERSION 5 " in hdr  # additive: the version stays
    dt = S.LIGHT_SHAPE
    assert dt.itemsize == 32 and dt.names == ("flags", "cos_outer", "cos_inner", "focus", "axis", "reserved")
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 28]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u\\n", '
                   "sizeof(skh_light_shape), offsetof(skh_light_shape, flags), offsetof(skh_light_shape, cos_outer), offsetof(skh_light_shape, cos_inner), "
                   "offsetof(skh_light_shape, focus), offsetof(skh_light_shape, axis), offsetof(skh_light_shape, reserved), sizeof(skh_light_shape_info), "
                   "SKH_LIGHT_SHAPE_SAMPLE_DISC, SKH_LIGHT_SHAPE_CONE, SKH_LSHAPE_PROBE_SAMPLE, SKH_LSHAPE_PROBE_PDF); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == [b"32", b"0", b"4", b"8", b"12", b"16", b"28", b"8", b"1", b"2", b"0", b"1"]
    assert (S.LIGHT_SHAPE_SAMPLE_DISC, S.LIGHT_SHAPE_CONE) == (1, 2) and capi.LIGHT_SHAPE_INFO.itemsize == 8
    assert capi.LSHAPE_PROBES == {"sample": (0, 6, 13), "pdf": (1, 7, 2)}


def test_the_header_is_a_dependency_of_the_build():
    deps = [os.path.basename(d) for d in build.DEPS]
    assert "skh_lshape.h" in deps
    # ... and so is every file the library's source tree includes
    csrc = os.path.join(ROOT, "strelka_amd", "csrc")
    for fn in os.listdir(csrc):
        for inc in re.findall(r'#include "([^"]+)"', open(os.path.join(csrc, fn)).read()):
            if os.path.exists(os.path.join(csrc, inc)):
                assert os.path.basename(inc) in deps, (fn, inc)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the header against the float64 statement
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lshape") / "skhlshape")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "strelka_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "skhlshape_main.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=60)
        assert out.returncode == 0, out.stderr
        return [ln.split() for ln in out.stdout.decode().splitlines()]

    return run


def hx(v):
    return " ".join("%08x" % int(x) for x in np.atleast_1d(np.asarray(v, F)).view(np.uint32))


def fl(word):
    return np.array([int(word, 16)], np.uint32).view(F)[0]


POW_ULP = 3.8  # skh_libm.h's stated pow error, in ulps


def test_cone_falloff_equals_the_reference(program):
    """s(c) over a fixed grid: c just below, equal to and just above cos_outer, equal to cos_inner, in between and at 1; a hard edge and a soft one; focus 0, 1
    and 7.5.  Both sides start from the same fp32 inputs.  The bar, relative, U = 2^-24 per rounding: the two differences are of floats -- one rounding each
    (none near the edge: Sterbenz) --, their quotient one: t carries 3 U; t t: 7 U; 3 - 2 t >= 1: 7 U; their product: 15 U; pow: 3.8 ulp = 7.6 U (skh_libm.h);
    the last product 1 U: 23.6 U with a focus, 15 U without.  Outside the cone, at its edge and on the plateau without focus the value is exact."""
    shapes = [(math.cos(math.radians(30)), None), (math.cos(math.radians(40)), math.cos(math.radians(20))), (math.cos(math.radians(25)), math.cos(math.radians(24.9))),
              (-0.5, 0.25)]
    lines, want, bars = [], [], []
    for co, ci in shapes:
        co = F(co)
        ci = co if ci is None else F(ci)
        cs = [np.nextafter(co, F(-2)), co, np.nextafter(co, F(2)), ci, np.nextafter(ci, F(-2)), np.nextafter(ci, F(2)), F(1.0), F(-1.0), F(0.0), F(1e-3)]
        cs += list(np.linspace(float(co), float(ci) if ci > co else 1.0, 41).astype(F))
        for focus in (0.0, 1.0, 7.5):
            for c in cs:
                lines.append("s " + hx([c, co, ci, focus]))
                want.append(float(lightref.s_cone(float(c), float(co), float(ci), focus)))
                bars.append((15 + (2 * POW_ULP + 1 if focus > 0 else 0)) * U)
    got = np.array([fl(r[0]) for r in program(lines)], np.float64)
    want, bars = np.array(want), np.array(bars)
    assert len(got) == len(want) == 4 * 3 * 51
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"s(c): worst |diff| / bar = {(rel / bars).max():.3f} over {len(got)} grid points ({int((want == 0).sum())} dark)")
    assert (got[want == 0] == 0).all() and (got[want > 0] > 0).all()
    assert (rel <= bars).all()
    # the plateau: t = 1 exactly from cos_inner on, the value is then pow alone (1 without a focus)
    assert float(fl(program(["s " + hx([1.0, 0.5, 0.75, 0.0])])[0][0])) == 1.0 and float(fl(program(["s " + hx([0.75, 0.5, 0.75, 0.0])])[0][0])) == 1.0
    assert float(fl(program(["s " + hx([np.nan, 0.5, 0.75, 0.0])])[0][0])) == 0.0


def test_sector_mapping_equals_the_reference(program):
    """k = min(int(16 ux), 15) and u' = 16 ux - k are EXACT in fp32: every boundary j / 16, its two neighbours, the ends of [0, 1] and a scrambled grid"""
    j = np.arange(17) / 16.0
    ux = np.concatenate([j, np.nextafter(j.astype(F), F(-1)), np.nextafter(j.astype(F), F(2)), (np.arange(4096) + 0.5) / 4096,
                         np.random.RandomState(3).rand(4096)]).astype(F)
    ux = ux[(ux >= 0) & (ux <= 1)]
    got = program(["k " + hx(u) for u in ux])
    k, up = lightref.sector(ux.astype(np.float64))
    assert np.array_equal(np.array([int(r[0]) for r in got]), k)
    assert np.array_equal(np.array([fl(r[1]) for r in got], np.float64), up)  # no rounding at all
    assert (up >= 0).all() and (up[ux < 1] < 1).all() and up[ux == 1][0] == 1.0  # (the sampler's draws are below 1)
    assert np.array_equal(np.bincount(k[-8192:-4096], minlength=16), np.full(16, 256))


def test_disc_point_equals_the_reference(program):
    """three discs (a small one, one under a rotation about a skew axis, one far from the origin).  The bar per coordinate, M = |O|_inf + |X|_inf + |Y|_inf
    (every vertex coordinate is at most that): a vertex carries the rounded cosine and sine, two products and two sums: 4 U M; the mapping three weights of
    <= 3 U absolute each, three products and two sums: 12 U M (tests/test_gpu_emit.py::test_probe_values): 16 U M.  The area: the cross product's
    components 3 U of |X|_1 |Y|_1 each (kappa), three squares, two sums, the root, the constant and the product: (kappa + 6) U."""
    rs = np.random.RandomState(5)
    R = S.rotate((0.3, -0.8, 0.52), 1.1)[:3, :3]
    discs = [((0.1, 1.5, -0.2), np.array([0.05, 0, 0]), np.array([0, 0, 0.05])), ((0.3, 2.0, 0.1), R @ [0.45, 0, 0], R @ [0, 0.45, 0]),
             ((1e3, 5.0, -1e3), np.array([5.0, 0, 0]), np.array([0, 0, -5.0]))]
    for O, X, Y in discs:
        O, X, Y = (np.asarray(v, F) for v in (O, X, Y))
        ux = np.concatenate([(np.arange(512) + 0.5) / 512, [0.0, 0.99999994]]).astype(F)
        uy = np.concatenate([rs.rand(512), [0.0, 0.99999994]]).astype(F)
        got = program(["p " + " ".join([hx(a), hx(b_), hx(O), hx(X), hx(Y)]) for a, b_ in zip(ux, uy)])
        O64, X64, Y64 = (v.astype(np.float64) for v in (O, X, Y))
        want = lightref.disc_point(O64, X64, Y64, ux.astype(np.float64), uy.astype(np.float64))
        pts = np.array([[fl(w) for w in r[1:4]] for r in got], np.float64)
        M = np.abs(O64).max() + np.abs(X64).max() + np.abs(Y64).max()
        err = np.abs(pts - want).max() / M
        area, want_a = float(fl(got[0][4])), lightref.disc_area(X64, Y64)
        kappa = np.abs(X64).sum() * np.abs(Y64).sum() / np.linalg.norm(np.cross(X64, Y64)) * 3
        print(f"disc |O| {np.abs(O64).max():g}: point {err / U:.2f} U M (bar 16), area {abs(area / want_a - 1) / U:.2f} U (bar {kappa + 6:.1f})")
        assert np.array_equal(np.array([int(r[0]) for r in got]), lightref.sector(ux.astype(np.float64))[0])
        assert err <= 16 * U and abs(area / want_a - 1) <= (kappa + 6) * U
        # inside the 16-gon: on its plane and on the inner side of the sector's rim edge
        n = np.cross(X64, Y64)
        n /= np.linalg.norm(n)
        assert np.abs((pts - O64) @ n).max() <= 16 * math.sqrt(3) * U * M


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference against Lambert's formula
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_quadrature_against_lamberts_formula():
    """the pure integrand cos_s cos_l / d^2 over the 16-gon against emitref.polygon_irradiance (E / Le, the same integral in
    closed form).  Midpoint rule over 16 x 24^2 cells of a smooth integrand: the error falls with the square of the cell size -- (r / 24 / d)^2 ~ 2e-4
    relative at d = 1.5 r = 0.5 with a constant of order 1; asserted at 5e-4, and halving the cells must quarter it."""
    O, X, Y = np.array([0.0, 1.5, 0.0]), np.array([0.5, 0.0, 0.0]), np.array([0.0, 0.0, -0.5])  # X x Y = +0.25 (0, 1, 0) -> n below
    n = np.array([0.0, -1.0, 0.0])
    poly = lightref.disc_vertices(O, X, Y)[:-1]
    assert abs(lightref.disc_area(X, Y) - 0.5 * sum(np.linalg.norm(np.cross(poly[k] - O, poly[(k + 1) % 16] - O)) for k in range(16))) < 1e-12
    for p in ((0.0, 0.0, 0.0), (2.2, 0.0, 1.0), (0.3, 0.0, -0.4)):
        want = emitref.polygon_irradiance(poly, np.array(p), (0, 1, 0))
        errs = []
        for m in (12, 24):
            pts, dA = lightref.disc_cells(O, X, Y, m)
            assert abs(dA.sum() - lightref.disc_area(X, Y)) < 1e-12
            errs.append(abs(lightref.irradiance_quadrature(pts, dA, n, p, (0, 1, 0)) / want - 1))
        print(f"p {p}: E / Le {want:.6f}, quadrature off by {errs[0]:.2e} (m 12), {errs[1]:.2e} (m 24)")
        assert errs[1] <= 5e-4 and errs[1] <= 0.3 * errs[0] + 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the scene layer
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_create_light_keys():
    sc = S.Scene()
    sc.createLight({"type": 0, "xform": S.translate((0, 2, 0)) @ S.rotate((1, 0, 0), math.radians(-90)), "useXform": True, "width": 1.0, "height": 0.5})
    assert "light_shapes" not in sc.arrays()  # no key without a shape
    assert "light_shapes" not in scenes.light_zoo().arrays()
    xf = S.translate((1, 2, 0)) @ S.rotate((1, 0, 0), math.radians(90))
    sc.createLight({"type": 1, "xform": xf, "useXform": True, "radius": 0.5, "sample": True})
    sc.createLight({"type": 1, "xform": xf, "useXform": True, "radius": 0.5, "coneAngle": math.radians(25.0)})
    sc.createLight({"type": 2, "xform": S.translate((0, 1, 0)) @ S.rotate((1, 0, 0), math.radians(-90)), "useXform": True, "radius": 0.1,
                    "coneAngle": math.radians(30.0), "coneSoftness": 0.5, "focus": 2.0})
    sc.createLight({"type": 0, "xform": S.translate((0, 2, 0)) @ S.rotate((1, 0, 0), math.radians(-90)), "useXform": True, "width": 1.0, "height": 0.5,
                    "coneAngle": math.radians(40.0), "axis": (0.0, -3.0, 4.0)})
    a = sc.arrays()
    ls = a["light_shapes"]
    assert ls.dtype == S.LIGHT_SHAPE and len(ls) == len(a["lights"]) == 5
    assert list(ls["flags"]) == [0, 1, 2, 2, 2] and (ls["reserved"] == 0).all()
    # defaults per type: a disk's normal (local +Z, here world -Y), a sphere's xform * (0, 0, -1) (here world -Y too), a rect's emission normal
    assert np.allclose(ls["axis"][2], (0, -1, 0), atol=1e-6) and np.allclose(ls["axis"][3], (0, -1, 0), atol=1e-6)
    L = a["lights"][4]["points"][:, :3].astype(np.float64)
    nrm = -np.cross(L[1] - L[0], L[3] - L[0])
    assert np.allclose(ls["axis"][4], (0, -0.6, 0.8), atol=1e-6) and np.allclose(nrm / np.linalg.norm(nrm), (0, -1, 0), atol=1e-6)
    # cos_inner from the softness: cos(angle (1 - softness)); a hard edge has cos_inner == cos_outer
    assert ls["cos_outer"][3] == F(math.cos(math.radians(30.0))) and ls["cos_inner"][3] == F(math.cos(math.radians(15.0))) and ls["focus"][3] == 2.0
    assert ls["cos_outer"][2] == ls["cos_inner"][2] == F(math.cos(math.radians(25.0))) and ls["focus"][2] == 0.0
    assert np.abs(np.linalg.norm(ls["axis"][2:].astype(np.float64), axis=1) - 1).max() < 1e-6
    with pytest.raises(ValueError):
        S.Scene().createLight({"type": 2, "radius": 0.1, "sample": True})
    with pytest.raises(ValueError):
        S.Scene().createLight({"type": 3, "halfAngle": 0.1, "coneAngle": 0.3})
    # spot_room: light_zoo's room, its three lights shaped
    sr = scenes.spot_room().arrays()
    zoo = scenes.light_zoo(with_rect=False).arrays()
    assert list(sr["lights"]["type"]) == [2, 1, 0] and list(sr["light_shapes"]["flags"]) == [2, 1, 2]
    assert np.array_equal(sr["vertices"][:len(zoo["vertices"])], zoo["vertices"]) and np.array_equal(sr["lights"][:2], zoo["lights"])
    scene_io.validate(sr)


def test_skscene_round_trip(tmp_path):
    sc = scenes.spot_room()
    arr = sc.arrays()
    p = str(tmp_path / "spot.skscene")
    scene_io.save_scene(p, arr, sc.getCamera())
    assert b"LSHP" in open(p, "rb").read()
    back = scene_io.load_scene(p).arrays()
    assert back["light_shapes"].dtype == S.LIGHT_SHAPE and np.array_equal(back["light_shapes"], arr["light_shapes"])
    assert np.array_equal(back["lights"], arr["lights"])
    zoo = scenes.light_zoo()
    q = str(tmp_path / "zoo.skscene")
    scene_io.save_scene(q, zoo.arrays(), zoo.getCamera())
    assert b"LSHP" not in open(q, "rb").read()
    assert "light_shapes" not in scene_io.load_scene(q).arrays()  # a file without the section loads as before
