"""CPU-side checks of emissive meshes' plumbing: the three C-ABI symbols and their Python binding, `Scene.addMaterial(emission=)` / `arrays()`,
the ingest paths (UsdPreviewSurface, OmniPBR, glTF emissiveFactor + KHR_materials_emissive_strength, the C++ twin in integration/SkhMaterials.h),
and the float64 restatement the GPU tests compare against (tests/emitref.py) against quadrature and a closed form."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import gltf, scene_io, scenes
from tests import emitref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emission_symbols_are_declared_exported_and_bound():
    from strelka_amd import build, capi

    build.build()
    lib = capi.load()
    text = open(os.path.join(ROOT, "include", "strelka_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("skh_set_emission", "skh_get_emitter_info", "skh_emitter_probe"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert "typedef struct skh_emitter_info" in header and "#define SKH_ABI_VERSION 5" in header
    assert re.search(r"#define SKH_EMIT_PROBE_SAMPLE 0u\s*#define SKH_EMIT_PROBE_PDF 1u", header) and "#define SKH_EMIT_MAX_ENTRIES (1u << 24)" in header
    assert capi.EMITTER_INFO.itemsize == 32 and capi.EMIT_PROBES == {"sample": (0, 6, 13), "pdf": (1, 8, 4)}
    # the option is documented in the option block
    assert re.search(r"emit_nee 1\|0", text)
    # a null context is refused by every one of them (SKH_INVALID_ARGUMENT = 3), without a GPU
    le = np.ones(3, np.float32)
    info = np.zeros((), capi.EMITTER_INFO)
    assert lib.skh_set_emission(None, le.ctypes.data_as(C.c_void_p), 1) == 3
    assert lib.skh_get_emitter_info(None, info.ctypes.data_as(C.c_void_p)) == 3
    assert lib.skh_emitter_probe(None, 0, None, 0, None) == 3
    assert lib.skh_set_option(None, b"emit_nee", 1) == 3


def test_the_table_header_is_a_dependency_of_the_library():
    from strelka_amd import build

    assert os.path.join(os.path.dirname(build.SRC), "skh_emit.h") in build.DEPS


def test_scene_arrays_carry_emission_only_when_a_material_emits():
    sc = scenes.cornell_box()
    keys = set(sc.arrays().keys())
    assert "emission" not in keys
    n = len(sc.arrays()["materials"])
    a = sc.addMaterial(S.MAT_DIFFUSE, (0, 0, 0), emission=(0.0, 0.0, 0.0))  # zero: does not emit
    assert set(sc.arrays().keys()) == keys
    b = sc.addMaterial(S.MAT_DIFFUSE, (0, 0, 0), emission=(5.0, 4.0, 0.5))
    h = sc.addHairMaterial(emission=(0.25, 0.0, 0.0))
    arr = sc.arrays()
    assert set(arr.keys()) == keys | {"emission"} and (a, b, h) == (n, n + 1, n + 2)
    em = arr["emission"]
    assert em.dtype == np.float32 and em.shape == (len(arr["materials"]), 3)
    assert np.array_equal(em[b], np.float32([5, 4, 0.5])) and np.array_equal(em[h], np.float32([0.25, 0, 0])) and not em[:b].any()
    for bad in ((1.0, -1.0, 0.0), (float("nan"), 0, 0), (float("inf"), 0, 0), (1.0, 2.0)):
        with pytest.raises(ValueError):
            sc.addMaterial(emission=bad)


def P(name, typ, value):
    return {"name": name, "type": typ, "value": value}


CASES = [
    ({"file": "", "name": "UsdPreviewSurface", "params": [P("diffuseColor", "float3", [0.2, 0.4, 0.6]), P("emissiveColor", "float3", [3.0, 2.0, 0.5])]}, (3.0, 2.0, 0.5)),
    ({"file": "", "name": "UsdPreviewSurface", "params": [P("emissiveColor", "float3", [0.0, 7.5, 0.0])]}, (0.0, 7.5, 0.0)),
    ({"file": "", "name": "UsdPreviewSurface", "params": [P("diffuseColor", "float3", [0.2, 0.4, 0.6])]}, (0.0, 0.0, 0.0)),
    ({"file": "OmniPBR.mdl", "name": "OmniPBR", "params": [P("enable_emission", "bool", True), P("emissive_color", "float3", [1.0, 0.5, 0.25]), P("emissive_intensity", "float", 40.0)]}, (40.0, 20.0, 10.0)),
    ({"file": "OmniPBR.mdl", "name": "OmniPBR", "params": [P("enable_emission", "bool", False), P("emissive_color", "float3", [1.0, 0.5, 0.25]), P("emissive_intensity", "float", 40.0)]}, (0.0, 0.0, 0.0)),
    ({"file": "OmniPBR.mdl", "name": "OmniPBR", "params": [P("emissive_color", "float3", [1.0, 0.5, 0.25]), P("emissive_intensity", "float", 40.0)]}, (0.0, 0.0, 0.0)),
    ({"file": "OmniPBR.mdl", "name": "OmniPBR", "params": [P("enable_emission", "bool", True)]}, (1.0, 1.0, 1.0)),
    ({"file": "OmniPBR.mdl", "name": "OmniPBR", "params": [P("enable_emission", "bool", True), P("emissive_color", "float3", [1.0, -0.5, 0.25])]}, (1.0, 0.0, 0.25)),
    ({"file": "OmniGlass.mdl", "name": "OmniGlass", "params": [P("enable_emission", "bool", True), P("emissive_color", "float3", [1.0, 1.0, 1.0])]}, (0.0, 0.0, 0.0)),
    ({"file": "default.mdl", "name": "default_material", "params": [P("diffuse_color", "float3", [0.3, 0.5, 0.7])]}, (0.0, 0.0, 0.0)),
]


def test_emission_from_description():
    for desc, want in CASES:
        got = scene_io.emission_from_description(desc)
        assert got.dtype == np.float32 and np.array_equal(got, np.float32(want)), (desc, got)
        # the material record is what it was: emission travels beside it
        assert np.array_equal(scene_io.material_from_description(desc), scene_io.material_from_description({**desc, "params": [p for p in desc["params"] if "emissi" not in p["name"] or p["name"] == "emissiveColor"]}))
    assert scene_io.emission_from_descriptions([c for c, _ in CASES[2:3]]) is None
    em = scene_io.emission_from_descriptions([c for c, _ in CASES])
    assert em.shape == (len(CASES), 3) and np.array_equal(em, np.float32([w for _, w in CASES]))


def test_cpp_emission_equals_the_python_statement(tmp_path):
    """integration/SkhMaterials.h skhmat::emission on a local look-alike of the reference's structs (tests/cpp/skhemission_main.cpp), case by case"""
    T = {"float": 0, "int": 1, "bool": 2, "float2": 3, "float3": 4, "float4": 5, "texture": 6}
    lines = []
    for c, _ in CASES:
        lines.append("D %s|%s|%d" % (c["file"], c["name"], len(c["params"])))
        for p_ in c["params"]:
            raw = bytes([1 if p_["value"] else 0]) if p_["type"] == "bool" else np.asarray(p_["value"], np.float32).tobytes()
            lines.append("P %d %s %s" % (T[p_["type"]], p_["name"], raw.hex() or "-"))
    exe = str(tmp_path / "skhemit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "skhemission_main.cpp")])
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = np.frombuffer(out.stdout, np.float32).reshape(-1, 3)
    assert np.array_equal(got, np.float32([scene_io.emission_from_description(c) for c, _ in CASES]))


def _write_gltf(path, materials):
    pos = np.float32([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    idx = np.uint16([0, 1, 2])
    blob = pos.tobytes() + idx.tobytes() + b"\0\0"
    open(os.path.join(os.path.dirname(path), "tri.bin"), "wb").write(blob)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": list(range(len(materials)))}],
           "nodes": [{"mesh": k} for k in range(len(materials))],
           "meshes": [{"primitives": [{"attributes": {"POSITION": 0}, "indices": 1, "material": k}]} for k in range(len(materials))],
           "materials": materials, "buffers": [{"uri": "tri.bin", "byteLength": len(blob)}],
           "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 6}],
           "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3", "min": [0, 0, 0], "max": [1, 1, 0]},
                         {"bufferView": 1, "componentType": 5123, "count": 3, "type": "SCALAR"}]}
    json.dump(doc, open(path, "w"))


def test_gltf_emissive_factor_and_strength(tmp_path):
    path = str(tmp_path / "lamp.gltf")
    plain = {"pbrMetallicRoughness": {"baseColorFactor": [0.5, 0.5, 0.5, 1.0]}}
    _write_gltf(path, [plain, {**plain, "emissiveFactor": [1.0, 0.5, 0.0], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 8.0}}},
                       {**plain, "emissiveFactor": [0.25, 0.25, 0.25]}, {**plain, "emissiveFactor": [0.0, 0.0, 0.0], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 8.0}}}])
    sc = gltf.load_gltf(path)
    d = sc.material_descriptions
    names = [[p["name"] for p in m["params"]] for m in d]
    assert names[0] == names[3] == ["diffuse_color_constant", "reflection_roughness_constant", "metallic_constant"]  # a zero factor: the description of before
    assert names[1] == names[0] + ["enable_emission", "emissive_color", "emissive_intensity"]
    arr = sc.arrays()
    assert np.array_equal(arr["emission"], np.float32([(0, 0, 0), (8, 4, 0), (0.25, 0.25, 0.25), (0, 0, 0)]))
    _write_gltf(path, [plain, plain])
    assert "emission" not in gltf.load_gltf(path).arrays()


def test_lambert_polygon_formula_against_quadrature():
    """the 1.0 x 0.6 quad at height 1.5 facing down, three floor points.  A 2000^2 midpoint rule carries its own h^2 error -- 2.0e-8 relative under the
    quad's centre --, so the formula is held against the Richardson extrapolation (4 Q(1000) - Q(500)) / 3 of the rule, whose error is O(h^4) ~ 1e-13 for this
    smooth integrand: 1e-10 relative, and the plain rule's distance from the formula must BE its h^2 term (it falls by 4 when h halves)."""
    quad = np.array([(-0.5, 1.5, -0.3), (0.5, 1.5, -0.3), (0.5, 1.5, 0.3), (-0.5, 1.5, 0.3)])
    for p in ((0.0, 0.0, 0.0), (2.0, 0.0, 1.0), (0.3, 0.0, -0.2)):
        a = emitref.polygon_irradiance(quad, p, (0, 1, 0))
        q = [emitref.quad_irradiance_quadrature(quad[0], quad[1] - quad[0], quad[3] - quad[0], p, (0, 1, 0), m) for m in (500, 1000)]
        assert abs(a / ((4 * q[1] - q[0]) / 3) - 1) <= 1e-10, (p, a, q)
        assert abs((q[0] - a) / (q[1] - a) - 4) <= 1e-3, (p, a, q)
    # split into triangles the formula is additive
    a = emitref.polygon_irradiance(quad, (2, 0, 1), (0, 1, 0))
    assert abs(emitref.polygon_irradiance(quad[[0, 1, 2]], (2, 0, 1), (0, 1, 0)) + emitref.polygon_irradiance(quad[[0, 2, 3]], (2, 0, 1), (0, 1, 0)) - a) <= 1e-15
    # far away the quad is a small source: E / Le -> A cos cos' / r^2
    p = np.array([30.0, 0.0, 40.0])
    r = np.linalg.norm(np.array([0, 1.5, 0]) - p)
    assert abs(emitref.polygon_irradiance(quad, p, (0, 1, 0)) / (0.6 * (1.5 / r) ** 2 / r ** 2) - 1) <= 1e-3


def test_one_triangle_closed_form():
    """One triangle: the table is {area * lum}, every draw selects entry 0, the points are uniform (their mean is the centroid, the sub-triangle nearest
    v0 at half scale holds a quarter of them), and the pdf integrates to 1: the mean of 1 / pdf over uniform points is the solid angle, which for a
    small far triangle is A cos / r^2, and E[cos_p / pdf] is Lambert's formula."""
    tri = np.array([[(0.0, 2.0, 0.0), (1.0, 2.0, 0.0), (0.0, 2.0, 1.0)]])  # winding: the normal points down, to the origin's side
    Le = np.float32([2.0, 1.0, 0.5])
    lum = emitref.lum709(Le)
    w, cdf, total = emitref.table(tri, [lum])
    assert abs(w[0] - 0.5 * lum) <= 1e-15 and cdf[-1] == 1.0 and abs(total - 0.5 * lum) <= 1e-15
    assert (emitref.select(cdf, [0.0, 0.5, 0.99999994]) == 0).all()
    n = emitref.normal(tri[0])
    assert np.allclose(n, (0, -1, 0)) and np.allclose(emitref.normal(tri[0], True), (0, 1, 0))
    m = 1024
    ux, uy = np.meshgrid((np.arange(m) + 0.5) / m, (np.arange(m) + 0.5) / m, indexing="ij")
    x = emitref.point(tri[0], ux.ravel(), uy.ravel())
    assert np.abs(x.mean(0) - tri[0].mean(0)).max() <= 1e-6
    assert abs(((x[:, 0] + x[:, 2]) <= 0.5).mean() - 0.25) <= 2e-3
    P0 = np.array([0.1, 0.0, 0.2])
    pd = emitref.pdf(n, lum, total, x, P0)
    assert (pd > 0).all() and (emitref.pdf(-n, lum, total, x, P0) == 0).all()
    d = x - P0
    cos_p = d[:, 1] / np.linalg.norm(d, axis=1)
    assert abs((cos_p / pd).mean() / emitref.polygon_irradiance(tri[0], P0, (0, 1, 0)) - 1) <= 1e-5
    far = np.array([0.0, -98.0, 0.0])
    assert abs((1 / emitref.pdf(n, lum, total, x, far)).mean() / (0.5 / 100.0 ** 2) - 1) <= 1e-2


def test_selection_restated():
    rs = np.random.RandomState(3)
    tris = rs.rand(50, 3, 3)
    lum = np.where(np.arange(50) % 7 == 0, 0.0, 1.0 + rs.rand(50))
    w, cdf, total = emitref.table(tris, lum)
    u = (np.arange(1 << 16) + 0.5) / (1 << 16)
    k = emitref.select(cdf, u)
    assert (w[k] > 0).all()  # an entry of weight 0 is never selected
    counts = np.bincount(k, minlength=50)
    assert np.abs(counts / len(u) - w / total).max() <= 2.0 / len(u)
