"""Material textures off the GPU ("Material textures"): the checker's look-up against the CPU oracle's, bit for bit; the mapping of
OmniPBR descriptions to skh_material_textures entries in Python and in C++; the glTF loader's opt-in keyword; the .skscene round trip."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import gltf, png, scene as S, scene_io
from tests import mtexref
from tests.test_gltf import make_gltf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_size():
    assert S.MATERIAL_TEXTURES.itemsize == 48
    assert S.MATERIAL_TEXTURES.names[:6] == ("roughness_texture", "metallic_texture", "emission_texture", "roughness_channel", "metallic_channel", "emission_channel")


def uv_lattice(w, h):
    """negatives, values > 1, texel centres and texel edges of a w x h texture, and the points between them"""
    us = np.concatenate([np.arange(-2 * w, 3 * w + 1) / (2.0 * w), [-1.37, -0.01, 0.013, 0.49999, 0.731, 1.0001, 2.6]])
    vs = np.concatenate([np.arange(-2 * h, 3 * h + 1) / (2.0 * h), [-2.2, -0.3, 0.27, 0.99999, 1.5]])
    return np.stack(np.meshgrid(us, vs, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)


@pytest.mark.parametrize("shape", [(3, 5), (4, 4)])  # (rows, columns): the 5 x 3 texture and the 4 x 4 one
def test_lookup_equals_the_oracle_bit_for_bit(ork, shape):
    tex = np.random.RandomState(11 + shape[0]).randint(0, 256, shape + (4,)).astype(np.uint8)
    uv = uv_lattice(shape[1], shape[0])
    want = np.zeros((len(uv), 4), np.float32)
    ork.ork_tex_lookup(tex.ctypes.data_as(C.c_void_p), C.c_uint32(tex.shape[1]), C.c_uint32(tex.shape[0]), uv.ctypes.data_as(C.c_void_p), C.c_uint32(len(uv)),
                       want.ctypes.data_as(C.c_void_p))
    got = mtexref.lookup(tex, uv)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the float64 statement of the same filter agrees to rounding
    assert np.abs(mtexref.lookup64(tex, uv.astype(np.float64)) - got).max() <= 4 * 2.0 ** -24


def test_resolve_material_definition():
    """a hand-worked case: plateau texels make the look-up exact, so the affine form and the clamp are all that is left"""
    tex = np.zeros((4, 4, 4), np.uint8)
    tex[..., 1] = 255
    m = np.zeros((), S.MATERIAL)
    m["type"], m["base_color"], m["roughness"], m["metallic"] = S.MAT_PBR, (0.1, 0.2, 0.3), 0.6, 0.2
    e = np.zeros((), S.MATERIAL_TEXTURES)
    e["roughness_texture"] = e["metallic_texture"] = e["emission_texture"] = 1
    e["roughness_channel"], e["metallic_channel"], e["emission_channel"] = 1, 0, 1
    e["roughness_scale"], e["roughness_bias"], e["metallic_scale"], e["metallic_bias"] = 0.5, 0.25, 3.0, -1.0
    uv = np.float32([[0.3, 0.7]])
    o = mtexref.resolve_material(m, e, (2.0, 3.0, 4.0), [tex], uv)[0]
    assert np.array_equal(o, np.float32([0.1, 0.2, 0.3, 0.75, 0.0, 2.0, 3.0, 4.0]))
    e["emission_channel"] = mtexref.RGB
    assert np.array_equal(mtexref.resolve_material(m, e, (2.0, 3.0, 4.0), [tex], uv)[0, 5:], np.float32([0.0, 3.0, 0.0]))
    m["type"] = S.MAT_DIFFUSE  # roughness / metallic maps are a PBR matter; emission is not
    o = mtexref.resolve_material(m, e, (2.0, 3.0, 4.0), [tex], uv)[0]
    assert np.array_equal(o[3:5], np.float32([0.6, 0.2])) and np.array_equal(o[5:], np.float32([0.0, 3.0, 0.0]))
    e["emission_texture"] = 2  # beyond the list = none
    assert np.array_equal(mtexref.resolve_material(m, e, (2.0, 3.0, 4.0), [tex], uv)[0, 5:], np.float32([2.0, 3.0, 4.0]))


def pbr(params, name="OmniPBR", file="OmniPBR.mdl"):
    return {"file": file, "name": name, "params": params}


def P(name, type_, value):
    return {"name": name, "type": type_, "value": value}


def entry(**kw):
    e = np.zeros((), S.MATERIAL_TEXTURES)
    e["emission_channel"], e["roughness_scale"], e["metallic_scale"] = 4, 1.0, 1.0
    for k, v in kw.items():
        e[k] = v
    return e


F = np.float32
# texture parameters carry uris here ("1" ... "4"), resolved through TEXIDS -- the form the glTF loader and the C++ side use; plain ids work too (below)
TEXIDS = {"1": 1, "2": 2, "3": 3, "4": 4}
CASES = [
    # influence 0: the map has no say, nothing is bound
    (pbr([P("reflection_roughness_constant", "float", 0.3), P("reflectionroughness_texture", "texture", "1"), P("reflection_roughness_texture_influence", "float", 0.0)]), entry()),
    # influence 0.5: scale = 0.5, bias = fl(constant * fl(1 - 0.5))
    (pbr([P("reflection_roughness_constant", "float", 0.3), P("reflectionroughness_texture", "texture", "2"), P("reflection_roughness_texture_influence", "float", 0.5),
          P("metallic_constant", "float", 0.7), P("metallic_texture", "texture", "3"), P("metallic_texture_influence", "float", 0.25)]),
     entry(roughness_texture=2, roughness_scale=0.5, roughness_bias=F(0.3) * F(0.5), metallic_texture=3, metallic_scale=0.25, metallic_bias=F(0.7) * F(0.75))),
    # influence 1: the texel alone
    (pbr([P("reflection_roughness_constant", "float", 0.3), P("reflectionroughness_texture", "texture", "1"), P("reflection_roughness_texture_influence", "float", 1.0)]),
     entry(roughness_texture=1, roughness_scale=1.0, roughness_bias=0.0)),
    # ORM: roughness = g, metallic = b of one texture, both influences 1; it wins over the standalone maps
    (pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", "4"), P("reflectionroughness_texture", "texture", "1"),
          P("reflection_roughness_texture_influence", "float", 1.0)]),
     entry(roughness_texture=4, metallic_texture=4, roughness_channel=1, metallic_channel=2)),
    # ORM with glTF's factors
    (pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", "2"), P("ORM_roughness_scale", "float", 0.8), P("ORM_metallic_scale", "float", 0.4)]),
     entry(roughness_texture=2, metallic_texture=2, roughness_channel=1, metallic_channel=2, roughness_scale=0.8, metallic_scale=0.4)),
    # ORM named but not enabled: nothing
    (pbr([P("enable_ORM_texture", "bool", False), P("ORM_texture", "texture", "4")]), entry()),
    # a mask against a colour texture: the colour texture wins, rgb
    (pbr([P("enable_emission", "bool", True), P("emissive_color", "float3", [1.0, 0.5, 0.25]), P("emissive_color_texture", "texture", "3"),
          P("emissive_mask_texture", "texture", "1")]), entry(emission_texture=3, emission_channel=4)),
    # the mask alone: channel r for all three
    (pbr([P("enable_emission", "bool", True), P("emissive_mask_texture", "texture", "1")]), entry(emission_texture=1, emission_channel=0)),
    # emission maps without enable_emission: nothing
    (pbr([P("emissive_color_texture", "texture", "3")]), entry()),
    # absent parameters
    (pbr([P("diffuse_color_constant", "float3", [0.5, 0.5, 0.5])]), entry()),
    # a texture that is not available (unknown uri): the slot binds nothing
    (pbr([P("reflectionroughness_texture", "texture", "9"), P("reflection_roughness_texture_influence", "float", 1.0)]), entry()),
    # non-PBR materials are ignored: glass, UsdPreviewSurface, the default material, hair
    (pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", "4")], "OmniGlass", "OmniGlass.mdl"), entry()),
    (pbr([P("diffuseColor", "float3", [0.2, 0.2, 0.2]), P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", "4")], "UsdPreviewSurface", "x.mtlx"), entry()),
    (pbr([P("enable_emission", "bool", True), P("emissive_mask_texture", "texture", "1")], "default_material", "default.mdl"), entry()),
    (pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", "4")], "hair", "hair.mdl"), entry()),
]


def test_description_mapping():
    for desc, want in CASES:
        got = scene_io.material_textures_from_description(desc, TEXIDS)
        assert got.dtype == S.MATERIAL_TEXTURES and got.tobytes() == want.tobytes(), (desc, got, want)
        # the material record and the emission are what they were: the maps travel beside them
        bare = {**desc, "params": [p for p in desc["params"] if p["type"] != "texture" and "ORM" not in p["name"] and "influence" not in p["name"]]}
        assert np.array_equal(scene_io.material_from_description(desc), scene_io.material_from_description(bare))
        assert np.array_equal(scene_io.emission_from_description(desc), scene_io.emission_from_description(bare))
    # plain 1-based ids in place of uris: what a .skscene description carries
    d = pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", 4)])
    assert scene_io.material_textures_from_description(d).tobytes() == CASES[3][1].tobytes()
    # the list: None when nothing is bound, else one entry per description
    assert scene_io.material_textures_from_descriptions([CASES[0][0], CASES[9][0]], TEXIDS) is None
    t = scene_io.material_textures_from_descriptions([c for c, _ in CASES], TEXIDS)
    assert t.shape == (len(CASES),) and t.tobytes() == b"".join(w.tobytes() for _, w in CASES)


def test_cpp_mapping_equals_the_python_statement(tmp_path):
    """integration/SkhMaterials.h skhmat::materialTextures on a local look-alike of the reference's structs (tests/cpp/skhmattex_main.cpp), case by case"""
    T = {"float": 0, "int": 1, "bool": 2, "float2": 3, "float3": 4, "float4": 5, "texture": 6}
    lines = []
    for c, _ in CASES:
        lines.append("D %s|%s|%d" % (c["file"], c["name"], len(c["params"])))
        for p_ in c["params"]:
            if p_["type"] == "bool":
                raw = bytes([1 if p_["value"] else 0])
            elif p_["type"] == "texture":
                raw = p_["value"].encode()
            else:
                raw = np.asarray(p_["value"], np.float32).tobytes()
            lines.append("P %d %s %s" % (T[p_["type"]], p_["name"], raw.hex() or "-"))
    exe = str(tmp_path / "skhmattex")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "skhmattex_main.cpp")])
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = np.frombuffer(out.stdout, S.MATERIAL_TEXTURES)
    # (the C++ side's texture ids are the decimal uris themselves; "9" is not available on the Python side and ORM-less case 10 binds nothing there: map it)
    want = np.array([scene_io.material_textures_from_description(c, {**TEXIDS, "9": 9}) for c, _ in CASES], S.MATERIAL_TEXTURES)
    assert len(got) == len(CASES) and got.tobytes() == want.tobytes()


def test_scene_arrays_carry_the_table_only_when_something_is_bound():
    sc = S.Scene()
    t = sc.addTexture(np.zeros((2, 2, 4), np.uint8))
    sc.addMaterial(S.MAT_PBR, (0.5, 0.5, 0.5))
    assert "material_textures" not in sc.arrays()
    sc.addMaterial(S.MAT_PBR, (0.5, 0.5, 0.5), roughness_texture=t, roughness_channel=1, roughness_scale=0.5, roughness_bias=0.25, metallic_texture=t, metallic_channel=2,
                   emission=(1.0, 2.0, 3.0), emission_texture=t, emission_channel=0)
    mt = sc.arrays()["material_textures"]
    assert mt.dtype == S.MATERIAL_TEXTURES and len(mt) == 2
    assert mt[0].tobytes() == entry().tobytes()
    assert mt[1].tobytes() == entry(roughness_texture=t, metallic_texture=t, emission_texture=t, roughness_channel=1, metallic_channel=2, emission_channel=0,
                                    roughness_scale=0.5, roughness_bias=0.25).tobytes()


def gltf_with_maps(tmp_path):
    path, _ = make_gltf(str(tmp_path))
    doc = json.load(open(path))
    doc["images"] += [{"uri": "orm.png"}, {"uri": "glow.png"}]
    doc["textures"] += [{"source": 1}, {"source": 2}]
    m = doc["materials"][0]
    m["pbrMetallicRoughness"]["metallicRoughnessTexture"] = {"index": 1}
    m["pbrMetallicRoughness"]["metallicFactor"] = 0.5
    m["emissiveFactor"] = [1.0, 0.5, 0.0]
    m["emissiveTexture"] = {"index": 2}
    doc["materials"][1]["pbrMetallicRoughness"]["metallicRoughnessTexture"] = {"index": 1}  # alphaMode BLEND -> OmniGlass: not read
    json.dump(doc, open(path, "w"))
    rs = np.random.RandomState(3)
    for name in ("albedo.png", "orm.png", "glow.png"):
        png.save_png(os.path.join(tmp_path, name), rs.randint(0, 256, (4, 4, 4)).astype(np.uint8))
    return path


def test_gltf_keyword_off_reproduces_todays_descriptions(tmp_path):
    path = gltf_with_maps(tmp_path)
    off = gltf.load_gltf(path)
    names = [[p["name"] for p in d["params"]] for d in off.material_descriptions]
    # exactly what the loader wrote before the keyword existed: the constants, the two textures it always read, the emission factor
    assert names == [["diffuse_color_constant", "reflection_roughness_constant", "metallic_constant", "diffuse_texture", "enable_emission", "emissive_color",
                      "emissive_intensity"], ["enable_opacity", "thin_walled", "frosting_roughness"]]
    arr = off.arrays()
    assert "material_textures" not in arr and len(arr["textures"]) == 1
    assert gltf.load_gltf(path, material_textures=False).material_descriptions == off.material_descriptions


def test_gltf_keyword_on_reads_the_maps(tmp_path):
    path = gltf_with_maps(tmp_path)
    on, off = gltf.load_gltf(path, material_textures=True), gltf.load_gltf(path)
    p = {x["name"]: x["value"] for x in on.material_descriptions[0]["params"]}
    assert p["enable_ORM_texture"] is True and p["ORM_texture"] == "orm.png" and p["ORM_roughness_scale"] == 0.4 and p["ORM_metallic_scale"] == 0.5
    assert p["emissive_color_texture"] == "glow.png"
    assert on.material_descriptions[1] == off.material_descriptions[1]  # the glass material: untouched
    arr = on.arrays()
    assert len(arr["textures"]) == 3
    ids = on.texture_ids
    mt = arr["material_textures"]
    assert mt[0].tobytes() == entry(roughness_texture=ids["orm.png"], metallic_texture=ids["orm.png"], roughness_channel=1, metallic_channel=2, roughness_scale=0.4,
                                    metallic_scale=0.5, emission_texture=ids["glow.png"], emission_channel=4).tobytes()
    assert mt[1].tobytes() == entry().tobytes()
    # everything else is what the keyword-off load gives
    a0 = off.arrays()
    assert arr["materials"].tobytes() == a0["materials"].tobytes() and np.array_equal(arr["emission"], a0["emission"])
    # a zero emissiveFactor: the texture scales nothing and is not read
    doc = json.load(open(path))
    doc["materials"][0]["emissiveFactor"] = [0.0, 0.0, 0.0]
    json.dump(doc, open(path, "w"))
    z = gltf.load_gltf(path, material_textures=True)
    assert "emissive_color_texture" not in [x["name"] for x in z.material_descriptions[0]["params"]] and int(z.arrays()["material_textures"][0]["emission_texture"]) == 0


def test_parameters_survive_the_skscene_round_trip(tmp_path):
    sc = S.Scene()
    for k in range(3):
        sc.addTexture(np.full((2, 3, 4), 40 * k, np.uint8))
    descs = [pbr([P("reflection_roughness_constant", "float", 0.3), P("reflectionroughness_texture", "texture", 2), P("reflection_roughness_texture_influence", "float", 0.5)]),
             pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", 3), P("enable_emission", "bool", True), P("emissive_color", "float3", [2.0, 1.0, 0.5]),
                  P("emissive_mask_texture", "texture", 1)])]
    for _ in descs:
        sc.addMaterial(S.MAT_PBR)
    vb = S.make_vertices([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [(0, 0), (1, 0), (0, 1)], [(1, 0, 0)] * 3)
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, np.arange(3)), 1, np.eye(4))
    arr = sc.arrays()
    want = scene_io.material_textures_from_descriptions(descs)
    assert want is not None
    for with_matl in (True, False):  # with the MATL section and with the descriptions alone
        a = dict(arr)
        if not with_matl:
            del a["materials"]
        p = os.path.join(tmp_path, "m%d.skscene" % with_matl)
        scene_io.save_scene(p, a, None, material_descriptions=descs)
        back = scene_io.load_scene(p)
        assert back.material_descriptions == descs
        assert back.arrays()["material_textures"].tobytes() == want.tobytes()
    # a map that names a texture the file does not hold is refused, as a base colour texture is
    bad = [pbr([P("enable_ORM_texture", "bool", True), P("ORM_texture", "texture", 7)]), descs[1]]
    p = os.path.join(tmp_path, "bad.skscene")
    scene_io.save_scene(p, arr, None, material_descriptions=bad)
    with pytest.raises(ValueError):
        scene_io.load_scene(p)
    # a file without such parameters loads without the key
    p = os.path.join(tmp_path, "plain.skscene")
    scene_io.save_scene(p, arr, None, material_descriptions=[pbr([]), pbr([])])
    assert "material_textures" not in scene_io.load_scene(p).arrays()
