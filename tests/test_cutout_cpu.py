"""Cutouts off the GPU ("Cutouts"): the reference loop of tests/cutref.py on a hand-made case with known answers (and, since the CPU checker
is at hand, masked = twin through it); the record's layout; the table in Scene.arrays(); the glTF, OmniPBR and UsdPreviewSurface mappings in Python and in
C++; the .skscene round trip; the GPU tests' ray grids stay inside their plateaus."""
import json
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import gltf, png, scene as S, scene_io
from tests import cutref
from tests.test_gltf import make_gltf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the record
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_record_size_and_offsets(tmp_path):
    dt = S.MATERIAL_CUTOUT
    assert dt.itemsize == 32
    assert dt.names == ("opacity_texture", "opacity_channel", "opacity_scale", "opacity_bias", "threshold", "reserved")
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # ... and the header's struct, through the host compiler
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(skh_material_cutout), offsetof(skh_material_cutout, opacity_texture), offsetof(skh_material_cutout, opacity_channel), "
                   "offsetof(skh_material_cutout, opacity_scale), offsetof(skh_material_cutout, opacity_bias), offsetof(skh_material_cutout, threshold), "
                   "offsetof(skh_material_cutout, reserved), sizeof(skh_cutout_info)); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == [b"32", b"0", b"4", b"8", b"12", b"16", b"20", b"40"]
    from strelka_amd import capi

    assert capi.CUTOUT_INFO.itemsize == 40


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference on a hand-made two-layer case
# ---------------------------------------------------------------------------------------------------------------------------------------------
def two_layers():
    """two 2 x 1 quads, uv 0..1 along x, at heights 1.0 (material 1) and 0.6 (material 2) over the floor; the half texture: left alpha 0 / red 0, right 255"""
    sc = S.Scene()
    tex = sc.addTexture(cutref.half_texture())
    for _ in range(3):
        sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    cutref.room(sc, 0)
    for y, mat in ((1.0, 1), (0.6, 2)):
        sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-1, y, 0.5), (1, y, 0.5), (1, y, -0.5), (-1, y, -0.5)], [(0, 1), (1, 1), (1, 0), (0, 0)]), mat, np.eye(4))
    return sc, tex


def test_reference_on_two_layers(ork):
    from tests import orklib

    sc, tex = two_layers()
    arr = sc.arrays()
    o = orklib.new_context()
    o.set_scene(arr)
    n = 8
    u = np.concatenate([np.linspace(0.15, 0.35, n), np.linspace(0.65, 0.85, n)])
    tg = np.stack([2 * u - 1, np.full(2 * n, 1.0), np.linspace(-0.3, 0.3, 2 * n)], -1)
    rays = cutref.make_rays(tg + np.array([0.0, 1.0, 0.0]), tg)  # straight down from height 2
    left, right = np.arange(n), np.arange(n, 2 * n)
    assert [int(i["type"]) for i in arr["instances"]] == [0, 0, 1, 0, 0]  # the floor, the wall, the light's proxy, the two layers
    floor, top, low = 0, 3, 4
    # (a) the top layer cut by alpha, the lower one by the INVERTED red channel: left rays pass the top and stop on the lower layer, right rays stop on the top
    tab = cutref.table(3, {1: cutref.entry(opacity_texture=tex, threshold=0.5), 2: cutref.entry(opacity_texture=tex, opacity_channel=0, opacity_scale=-1.0, opacity_bias=1.0, threshold=0.5)})
    h, info = cutref.trace(o, arr, tab, rays, 0, margin=1.5)
    assert (h["instance_id"][left] == low).all() and np.allclose(h["t"][left], 1.4, atol=1e-5)
    assert (h["instance_id"][right] == top).all() and np.allclose(h["t"][right], 1.0, atol=1e-5)
    assert info["continued"] == n and info["capped"] == 0 and info["first_cut"].tolist() == [True] * n + [False] * n
    # (b) both layers cut by alpha: left rays reach the floor after two rejections
    tab2 = cutref.table(3, {1: cutref.entry(opacity_texture=tex, threshold=0.5), 2: cutref.entry(opacity_texture=tex, threshold=1.0)})
    h, info = cutref.trace(o, arr, tab2, rays, 0, margin=1.5)
    assert (h["instance_id"][left] == floor).all() and np.allclose(h["t"][left], 2.0, atol=1e-5) and info["continued"] == 2 * n and info["per_round"][:2] == [n, n]
    # ... and with a round limit of 1 the second cut hit is accepted whatever its opacity
    h, info = cutref.trace(o, arr, tab2, rays, 0, rounds=1, margin=1.5)
    assert (h["instance_id"][left] == low).all() and info["continued"] == n and info["capped"] == n
    # shadow rays that end between the layers and the floor: occluded on the right only; reaching the floor: all
    sh = np.array(rays, copy=True)
    sh["tmax"] = 1.7
    s, _ = cutref.trace(o, arr, tab2, sh, 1, margin=1.5)
    assert (s["t"][left] == -1).all() and (s["t"][right] == 1).all()
    sh["tmax"] = 2.5
    s, _ = cutref.trace(o, arr, tab2, sh, 1, margin=1.5)
    assert (s["t"] == 1).all()
    s, info = cutref.trace(o, arr, tab2, sh, 1, rounds=1, margin=1.5)
    assert (s["t"] == 1).all() and info["capped"] == n
    # a constant opacity without a texture: bias alone decides
    for bias, cut in ((0.3, True), (0.5, False)):
        t3 = cutref.table(3, {1: cutref.entry(opacity_scale=0.0, opacity_bias=bias, threshold=0.5)})
        h, _ = cutref.trace(o, arr, t3, rays, 0)
        assert (h["instance_id"] == (low if cut else top)).all()
    # no table, or thresholds 0: the checker's own hits
    plain = o.trace(rays, 0)
    for t in (None, cutref.table(3, {})):
        h, info = cutref.trace(o, arr, t, rays, 0)
        assert h.tobytes() == plain.tobytes() and info["continued"] == 0
    # a footprint that leaves its plateau is an error, not a skipped ray
    bad = cutref.make_rays(np.float32([[0.0, 2.0, 0.0]]), np.float64([[0.0, 1.0, 0.0]]))  # u = 0.5: the border
    with pytest.raises(AssertionError):
        cutref.trace(o, arr, tab, bad, 0, margin=1.5)


@pytest.mark.parametrize("layout", ["single", "shared"])
def test_reference_masked_equals_twin_on_the_cpu(ork, layout):
    """the card scene through the CPU checker: the reference's hits on the masked scene are the checker's own on the twin (primitives through the kept map)"""
    from tests import orklib

    sc, tab, kept = cutref.card_scene(False, layout)
    tw, _, _ = cutref.card_scene(True, layout)
    arr, tarr = sc.arrays(), tw.arrays()
    o, ot = orklib.new_context(), orklib.new_context()
    o.set_scene(arr)
    ot.set_scene(tarr)
    cards = cutref.card_instances(arr)
    for oblique in (False, True):
        rays = cutref.card_rays(layout, oblique, 512)
        h, info = cutref.trace(o, arr, tab, rays, 0)
        want = ot.trace(rays, 0)
        on_card = np.isin(want["instance_id"], cards)
        prim = np.where(on_card, kept[np.minimum(want["prim_id"], len(kept) - 1)], want["prim_id"])
        for f in ("t", "u", "v", "instance_id"):
            assert np.array_equal(h[f], want[f]), f
        assert np.array_equal(h["prim_id"], prim)
        assert 0 < info["continued"] < len(rays) and info["continued"] == int(info["first_cut"].sum()) and on_card.any()
        sh = cutref.shadow_version(rays)
        s, _ = cutref.trace(o, arr, tab, sh, 1)
        assert np.array_equal(s["t"], ot.trace(sh, 1)["t"]) and (s["t"] == 1).any() and (s["t"] == -1).any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' grids stay inside their plateaus
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gpu_ray_grids_stay_inside_plateaus():
    from tests import test_gpu_cutout as G

    for layout, oblique, count in G.HIT_CASES:
        rays = cutref.card_rays(layout, oblique, count)
        assert len(rays) == count
        c = cutref.edge_clearance(rays, layout)
        assert np.isfinite(c).all() and c.min() > 0.01, (layout, oblique, count, c.min())  # every ray crosses a card, a hundredth of a cell from any edge at least
    # the block centres: the footprint is the block
    _, blocks, uv = cutref.card_triangles()
    tex = cutref.card_texture(cutref.block_alpha())
    assert cutref.footprint_is_plateau(tex, 3, uv, 0.25).all()
    assert sorted(set(blocks)) == [(a, b) for a in range(4) for b in range(4)]
    for a in (cutref.block_alpha(), cutref.block_alpha(flip=True)):
        k = cutref.card_kept(a)
        assert 4 <= k.sum() <= 28  # some kept, some cut
    # the interpolated-uv rays: two texels from the border at u = 0.5 and from the wrap
    rays, u = cutref.half_rays()
    assert ((np.abs(u - 0.5) >= 0.15 - 1e-12) & (u >= 0.15 - 1e-12) & (u <= 0.85 + 1e-12)).all()
    uv = np.stack([u, np.full(len(u), 0.5)], -1)
    for ch in (0, 3):
        assert cutref.footprint_is_plateau(cutref.half_texture(), ch, uv, 1.5).all()
    # the rays do cross the quad where they aim
    o, d = np.asarray(rays["origin"], np.float64), np.asarray(rays["dir"], np.float64)
    p = o + ((1.0 - o[:, 1]) / d[:, 1])[:, None] * d
    assert np.allclose((p[:, 0] + 1) / 2, u, atol=1e-6) and (np.abs(p[:, 2]) < 0.45).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Scene.addMaterial -> arrays()
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_scene_arrays_carry_the_table_only_when_a_material_is_a_cutout():
    sc = S.Scene()
    t = sc.addTexture(np.zeros((2, 2, 4), np.uint8))
    sc.addMaterial(S.MAT_PBR, (0.5, 0.5, 0.5))
    sc.addMaterial(S.MAT_PBR, (0.5, 0.5, 0.5), opacity_texture=t)  # a texture without a threshold: no cutout
    assert "material_cutouts" not in sc.arrays()
    sc.addMaterial(S.MAT_DIFFUSE, opacity_texture=t, opacity_threshold=0.25)
    sc.addMaterial(S.MAT_DIFFUSE, opacity_channel=0, opacity_scale=0.0, opacity_bias=0.75, opacity_threshold=1.0)
    ct = sc.arrays()["material_cutouts"]
    assert ct.dtype == S.MATERIAL_CUTOUT and len(ct) == 4
    assert ct[0].tobytes() == ct[1].tobytes() == cutref.entry().tobytes()
    assert ct[2].tobytes() == cutref.entry(opacity_texture=t, threshold=0.25).tobytes()
    assert ct[3].tobytes() == cutref.entry(opacity_channel=0, opacity_scale=0.0, opacity_bias=0.75, threshold=1.0).tobytes()
    for bad in (dict(opacity_threshold=1.5), dict(opacity_threshold=-0.1), dict(opacity_threshold=0.5, opacity_channel=4)):
        with pytest.raises(ValueError):
            sc.addMaterial(**bad)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# descriptions: OmniPBR, UsdPreviewSurface -- Python and C++
# ---------------------------------------------------------------------------------------------------------------------------------------------
def P(name, type_, value):
    return {"name": name, "type": type_, "value": value}


def desc(params, name="OmniPBR", file="OmniPBR.mdl"):
    return {"file": file, "name": name, "params": params}


TEXIDS = {"1": 1, "2": 2, "3": 3}
CASES = [
    # OmniPBR with a map: its alpha for opacity_mode 0 (the default) ...
    (desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "2"), P("opacity_threshold", "float", 0.5)]),
     cutref.entry(opacity_texture=2, threshold=0.5), S.MAT_PBR),
    # ... its red channel for the other modes (the stated simplification)
    (desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "3"), P("opacity_mode", "int", 1),
           P("opacity_threshold", "float", 0.25)]), cutref.entry(opacity_texture=3, opacity_channel=0, threshold=0.25), S.MAT_PBR),
    # glTF's factor rides on opacity_scale
    (desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "1"), P("opacity_mode", "int", 0),
           P("opacity_scale", "float", 0.8), P("opacity_constant", "float", 0.8), P("opacity_threshold", "float", 0.5)]),
     cutref.entry(opacity_texture=1, opacity_scale=0.8, threshold=0.5), S.MAT_PBR),
    # without a map: the constant alone (texel = 1 x scale 0)
    (desc([P("enable_opacity", "bool", True), P("opacity_constant", "float", 0.3), P("opacity_threshold", "float", 0.5)]),
     cutref.entry(opacity_scale=0.0, opacity_bias=0.3, threshold=0.5), S.MAT_PBR),
    # the map named but not enabled: the constant (OmniPBR.mdl's default 1)
    (desc([P("enable_opacity", "bool", True), P("opacity_texture", "texture", "2"), P("opacity_threshold", "float", 0.5)]),
     cutref.entry(opacity_scale=0.0, opacity_bias=1.0, threshold=0.5), S.MAT_PBR),
    # a map that is not available: likewise
    (desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "9"), P("opacity_constant", "float", 0.6),
           P("opacity_threshold", "float", 0.5)]), cutref.entry(opacity_scale=0.0, opacity_bias=0.6, threshold=0.5), S.MAT_PBR),
    # no threshold, or opacity not enabled: no cutout
    (desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "2")]), cutref.entry(), S.MAT_PBR),
    (desc([P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", "2"), P("opacity_threshold", "float", 0.5)]), cutref.entry(), S.MAT_PBR),
    # a threshold above 1 is clamped
    (desc([P("enable_opacity", "bool", True), P("opacity_constant", "float", 0.3), P("opacity_threshold", "float", 2.0)]),
     cutref.entry(opacity_scale=0.0, opacity_bias=0.3, threshold=1.0), S.MAT_PBR),
    # OmniGlass keeps its meaning of enable_opacity
    (desc([P("enable_opacity", "bool", True), P("opacity_threshold", "float", 0.5)], "OmniGlass", "OmniGlass.mdl"), cutref.entry(), S.MAT_GLASS),
    # UsdPreviewSurface: a threshold makes the opacity a cutout's -- and the material is NOT glass, even with an opacity below 0.5
    (desc([P("diffuseColor", "float3", [0.2, 0.3, 0.4]), P("opacity", "float", 0.3), P("opacityThreshold", "float", 0.5)], "UsdPreviewSurface", "x.mtlx"),
     cutref.entry(opacity_scale=0.0, opacity_bias=0.3, threshold=0.5), S.MAT_PBR),
    (desc([P("diffuseColor", "float3", [0.2, 0.3, 0.4]), P("opacityThreshold", "float", 0.1)], "UsdPreviewSurface", "x.mtlx"),
     cutref.entry(opacity_scale=0.0, opacity_bias=1.0, threshold=0.1), S.MAT_PBR),
    # ... without a threshold everything stays as it is: glass below 0.5
    (desc([P("diffuseColor", "float3", [0.2, 0.3, 0.4]), P("opacity", "float", 0.3)], "UsdPreviewSurface", "x.mtlx"), cutref.entry(), S.MAT_GLASS),
    (desc([P("diffuseColor", "float3", [0.2, 0.3, 0.4]), P("opacity", "float", 0.3), P("opacityThreshold", "float", 0.0)], "UsdPreviewSurface", "x.mtlx"), cutref.entry(), S.MAT_GLASS),
    # the default material, hair
    (desc([P("enable_opacity", "bool", True), P("opacity_threshold", "float", 0.5)], "default_material", "default.mdl"), cutref.entry(), S.MAT_DIFFUSE),
    (desc([P("enable_opacity", "bool", True), P("opacity_threshold", "float", 0.5)], "hair", "hair.mdl"), cutref.entry(), S.MAT_HAIR),
]


def test_description_mapping():
    for d, want, mtype in CASES:
        got = scene_io.material_cutout_from_description(d, TEXIDS)
        assert got.dtype == S.MATERIAL_CUTOUT and got.tobytes() == want.tobytes(), (d, got, want)
        assert int(scene_io.material_from_description(d)["type"]) == mtype, d
    # plain 1-based ids in place of uris: what a .skscene description carries
    d = desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", 2), P("opacity_threshold", "float", 0.5)])
    assert scene_io.material_cutout_from_description(d).tobytes() == CASES[0][1].tobytes()
    # the list: None when nothing is a cutout, else one entry per description
    assert scene_io.material_cutouts_from_descriptions([CASES[6][0], CASES[12][0]], TEXIDS) is None
    t = scene_io.material_cutouts_from_descriptions([c for c, _, _ in CASES], TEXIDS)
    assert t.shape == (len(CASES),) and t.tobytes() == b"".join(w.tobytes() for _, w, _ in CASES)


def test_cpp_mapping_equals_the_python_statement(tmp_path):
    """integration/SkhMaterials.h skhmat::materialCutout and skhmat::translate on a local look-alike of the reference's structs (tests/cpp/skhcutout_main.cpp)"""
    T = {"float": 0, "int": 1, "bool": 2, "float2": 3, "float3": 4, "float4": 5, "texture": 6}
    lines = []
    for c, _, _ in CASES:
        lines.append("D %s|%s|%d" % (c["file"], c["name"], len(c["params"])))
        for p_ in c["params"]:
            if p_["type"] == "bool":
                raw = bytes([1 if p_["value"] else 0])
            elif p_["type"] == "texture":
                raw = p_["value"].encode()
            elif p_["type"] == "int":
                raw = np.asarray(p_["value"], np.int32).tobytes()
            else:
                raw = np.asarray(p_["value"], np.float32).tobytes()
            lines.append("P %d %s %s" % (T[p_["type"]], p_["name"], raw.hex() or "-"))
    exe = str(tmp_path / "skhcutout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "skhcutout_main.cpp")])
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rec = np.dtype([("cut", S.MATERIAL_CUTOUT), ("mat", S.MATERIAL)])
    got = np.frombuffer(out.stdout, rec)
    assert len(got) == len(CASES)
    # (the C++ side's texture ids are the decimal uris themselves: "9" exists there)
    for k, (c, _, mtype) in enumerate(CASES):
        want = scene_io.material_cutout_from_description(c, {**TEXIDS, "9": 9})
        assert got["cut"][k].tobytes() == want.tobytes(), (k, got["cut"][k], want)
        assert int(got["mat"][k]["type"]) == mtype
        if mtype != S.MAT_HAIR:  # (the hair block's absorption goes through log() on both sides: tests/test_integration_files.py holds it to rounding)
            assert got["mat"][k].tobytes() == scene_io.material_from_description(c).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# glTF
# ---------------------------------------------------------------------------------------------------------------------------------------------
def gltf_with_masks(tmp_path):
    path, _ = make_gltf(str(tmp_path))
    doc = json.load(open(path))
    doc["materials"][0]["alphaMode"] = "MASK"  # baseColorTexture, factor alpha 1, no alphaCutoff: the default 0.5
    doc["materials"].append({"name": "grille", "alphaMode": "MASK", "alphaCutoff": 0.3, "pbrMetallicRoughness": {"baseColorFactor": [0.5, 0.5, 0.5, 0.7]}})
    json.dump(doc, open(path, "w"))
    png.save_png(os.path.join(tmp_path, "albedo.png"), np.random.RandomState(3).randint(0, 256, (4, 4, 4)).astype(np.uint8))
    return path


def test_gltf_alpha_mask(tmp_path):
    path = gltf_with_masks(tmp_path)
    off, on = gltf.load_gltf(path), gltf.load_gltf(path, alpha_mask=True)
    # the default keeps the reference loader's behaviour: every non-OPAQUE material is OmniGlass, nothing is a cutout
    assert [d["name"] for d in off.material_descriptions] == ["OmniGlass", "OmniGlass", "OmniGlass"]
    assert gltf.load_gltf(path, alpha_mask=False).material_descriptions == off.material_descriptions
    a0 = off.arrays()
    assert "material_cutouts" not in a0 and [int(t) for t in a0["materials"]["type"]] == [S.MAT_GLASS] * 3
    # with the keyword MASK becomes OmniPBR with a cutout; BLEND stays glass
    assert [d["name"] for d in on.material_descriptions] == ["OmniPBR", "OmniGlass", "OmniPBR"]
    assert on.material_descriptions[1] == off.material_descriptions[1]
    arr = on.arrays()
    tid = on.texture_ids["albedo.png"]
    assert [int(t) for t in arr["materials"]["type"]] == [S.MAT_PBR, S.MAT_GLASS, S.MAT_PBR]
    assert int(arr["materials"][0]["base_color_texture"]) == tid and np.allclose(arr["materials"][2]["base_color"], 0.5)
    ct = arr["material_cutouts"]
    assert len(ct) == 3
    assert ct[0].tobytes() == cutref.entry(opacity_texture=tid, opacity_channel=3, opacity_scale=1.0, opacity_bias=0.0, threshold=0.5).tobytes()  # the default alphaCutoff
    assert ct[1].tobytes() == cutref.entry().tobytes()
    assert ct[2].tobytes() == cutref.entry(opacity_scale=0.0, opacity_bias=F(0.7), threshold=F(0.3)).tobytes()  # no texture: the factor's alpha alone
    # a factor alpha below 1 scales the texel
    doc = json.load(open(path))
    doc["materials"][0]["pbrMetallicRoughness"]["baseColorFactor"] = [1.0, 1.0, 1.0, 0.6]
    doc["materials"][0]["alphaCutoff"] = 0.25
    json.dump(doc, open(path, "w"))
    ct = gltf.load_gltf(path, alpha_mask=True).arrays()["material_cutouts"]
    assert ct[0].tobytes() == cutref.entry(opacity_texture=tid, opacity_scale=F(0.6), threshold=0.25).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# .skscene
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_parameters_survive_the_skscene_round_trip(tmp_path):
    sc = S.Scene()
    for k in range(3):
        sc.addTexture(np.full((2, 3, 4), 40 * k, np.uint8))
    descs = [CASES[0][0], CASES[10][0], desc([])]
    descs[0] = desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", 2), P("opacity_threshold", "float", 0.5)])
    for _ in descs:
        sc.addMaterial(S.MAT_PBR)
    vb = S.make_vertices([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0, 1)], [(1, 0, 0)] * 3)
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, np.arange(3)), 1, np.eye(4))
    arr = sc.arrays()
    want = scene_io.material_cutouts_from_descriptions(descs)
    assert want is not None and (want["threshold"] > 0).tolist() == [True, True, False]
    for with_matl in (True, False):  # with the MATL section and with the descriptions alone
        a = dict(arr)
        if not with_matl:
            del a["materials"]
        p = os.path.join(tmp_path, "m%d.skscene" % with_matl)
        scene_io.save_scene(p, a, None, material_descriptions=descs)
        back = scene_io.load_scene(p)
        assert back.material_descriptions == descs
        assert back.arrays()["material_cutouts"].tobytes() == want.tobytes()
        if not with_matl:
            assert int(back.arrays()["materials"][1]["type"]) == S.MAT_PBR  # the UsdPreviewSurface cutout is not glass
    # an opacity map that names a texture the file does not hold is refused, as a base colour texture is
    bad = [desc([P("enable_opacity", "bool", True), P("enable_opacity_texture", "bool", True), P("opacity_texture", "texture", 7), P("opacity_threshold", "float", 0.5)])] + descs[1:]
    p = os.path.join(tmp_path, "bad.skscene")
    scene_io.save_scene(p, arr, None, material_descriptions=bad)
    with pytest.raises(ValueError):
        scene_io.load_scene(p)
    # a file without such parameters loads without the key
    p = os.path.join(tmp_path, "plain.skscene")
    scene_io.save_scene(p, arr, None, material_descriptions=[desc([]), desc([]), desc([])])
    assert "material_cutouts" not in scene_io.load_scene(p).arrays()
