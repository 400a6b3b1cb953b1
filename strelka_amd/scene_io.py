"""Flat binary scene dump (".skscene"): the arrays ``oka::Scene`` hands the renderer, written verbatim.

SURVEY.md section 8(f) N2: the reference reaches its scenes through OpenUSD / tinygltf, neither of which exists on the GPU
box.  Where Strelka builds, a ~40-line exporter (`Scene::saveDump` in strelka_amd/host is the same
code against this repository's mirror of the headers) writes what `OptiXRender::render()` uploads on its first frame
(OptixRender.cpp:876-888, getters of include/scene/scene.h:199-216 and :229-327); `bench.py --scene file.skscene` and
`load_scene()` consume it without any third-party dependency.

Layout (little endian)::

    header   : char magic[8] = "SKSCENE\\0"; u32 version = 1; u32 section_count
    section  : char tag[4]; u32 elem_size; u64 count; u8 data[elem_size * count]; zero padding to a multiple of 8

    tag   element                                        reference source
    VERT  32 B vertex {float3 pos; u32 tangent, normal, uv; 2 pad}   Scene::getVertices()            scene.h:80-89
    INDX  u32 mesh-local index                                        Scene::getIndices()
    MESH  4 x u32 {index_offset, index_count, vertex_offset, vertex_count}   Scene::getMeshes()      scene.h:21-27
    CPTS  float3 control point            Scene::getCurvesPoint()
    CWID  float radius                    Scene::getCurvesWidths()
    CVCN  u32 control points per strand   Scene::getCurvesVertexCounts()
    CURV  6 x u32                         Scene::getCurves()                                         scene.h:29-42
    INST  64 B {float m[12] (3x4 row-major = glm::float3x4(glm::rowMajor4(transform)), OptixRender.cpp:438);
                u32 type, geom_id, material_id, light_id}             Scene::getInstances()          scene.h:44-60
    LGHT  112 B UniformLight              Scene::getLights()                                         Lights.h / scene.h:146-155
    MATL  64 B skh_material (the fixed argument block MaterialDescription maps to)
    MDSC  u8 JSON text: the original MaterialDescription list [{"file", "name", "params": [{"name", "type", "value"}]}]
          (optional; `materials_from_descriptions` turns it into MATL when MATL is absent)
    CAMR  96 B {float view[16] (world -> view, row-major); float fov_deg, znear, zfar; u32 pad[5]}   Camera::matrices.view, fov
    TXDS  4 x u32 {offset (texels), width, height, 0} per texture; materials refer to texture k as id k + 1 (0 = none)
    TXEL  u32 RGBA8 texel (R in the low byte), rows top to bottom as stbi_load returns them (OptixRender.cpp:1191-1264)
Unknown tags are skipped, so the format can grow.
"""
import json
import struct

import numpy as np

from . import scene as S

MAGIC = b"SKSCENE\0"
VERSION = 1
CAMERA = np.dtype([("view", np.float32, 16), ("fov", np.float32), ("znear", np.float32), ("zfar", np.float32),
                   ("pad", np.uint32, 5)])
assert CAMERA.itemsize == 96

_SECTIONS = [  # tag, key in Scene.arrays(), dtype
    (b"VERT", "vertices", S.VERTEX),
    (b"INDX", "indices", np.dtype(np.uint32)),
    (b"MESH", "meshes", S.MESH),
    (b"CPTS", "curve_points", np.dtype((np.float32, 3))),
    (b"CWID", "curve_radii", np.dtype(np.float32)),
    (b"CVCN", "curve_vertex_counts", np.dtype(np.uint32)),
    (b"CURV", "curves", S.CURVE),
    (b"INST", "instances", S.INSTANCE),
    (b"LGHT", "lights", S.LIGHT),
    (b"MATL", "materials", S.MATERIAL),
]


def _camera_record(cam):
    rec = np.zeros(1, CAMERA)
    rec["view"][0] = np.asarray(cam.view, np.float64).astype(np.float32).reshape(16)
    rec["fov"], rec["znear"], rec["zfar"] = cam.fov, cam.znear, cam.zfar
    return rec


def save_scene(path, arrays, camera=None, material_descriptions=None):
    """arrays: the dict of Scene.arrays(); camera: scene.Camera (optional); material_descriptions: list of dicts (optional)."""
    sections = []
    for tag, key, dt in _SECTIONS:
        if key in arrays and arrays[key] is not None:
            a = np.ascontiguousarray(arrays[key], dtype=dt.base if dt.shape else dt)
            if dt.shape:
                a = a.reshape((-1,) + dt.shape)
            sections.append((tag, dt.itemsize, len(a), a.tobytes()))
    if arrays.get("textures"):
        desc, texels = S.pack_textures(arrays["textures"])
        sections.append((b"TXDS", S.TEXTURE_DESC.itemsize, len(desc), desc.tobytes()))
        sections.append((b"TXEL", 4, len(texels), texels.tobytes()))
    if arrays.get("material_blend") is not None and len(arrays["material_blend"]):
        # fractional opacity (skh_set_material_blend): a section of its own -- a reader that does not know the tag skips it, a file without it has no blend
        bt = np.ascontiguousarray(arrays["material_blend"], S.MATERIAL_BLEND).reshape(-1)
        sections.append((b"MBLD", S.MATERIAL_BLEND.itemsize, len(bt), bt.tobytes()))
    if arrays.get("light_shapes") is not None and len(arrays["light_shapes"]):
        # light shapes (skh_set_light_shapes): likewise a section of its own, written only when present
        ls = np.ascontiguousarray(arrays["light_shapes"], S.LIGHT_SHAPE).reshape(-1)
        sections.append((b"LSHP", S.LIGHT_SHAPE.itemsize, len(ls), ls.tobytes()))
    if material_descriptions is not None:
        text = json.dumps(material_descriptions).encode()
        sections.append((b"MDSC", 1, len(text), text))
    if camera is not None:
        sections.append((b"CAMR", CAMERA.itemsize, 1, _camera_record(camera).tobytes()))
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", VERSION, len(sections)))
        for tag, esz, cnt, data in sections:
            assert len(data) == esz * cnt
            f.write(tag + struct.pack("<IQ", esz, cnt) + data + b"\0" * (-len(data) % 8))


class LoadedCamera(S.Camera):
    """oka::Camera restored from its view matrix (position / orientation are not needed by the renderer)."""

    def __init__(self, view, fov, znear, zfar):
        super().__init__(fov=fov, znear=znear, zfar=zfar, name="dumped camera")
        self.view = np.asarray(view, np.float64).reshape(4, 4)

    def updateViewMatrix(self):
        pass


class LoadedScene:
    """Duck-types strelka_amd.scene.Scene for the consumers (arrays(), getCamera())."""

    def __init__(self, arrays, cameras, material_descriptions=None):
        self._arrays = arrays
        self.mCameras = cameras
        self.material_descriptions = material_descriptions

    def arrays(self):
        return self._arrays

    def getCamera(self, index=0):
        return self.mCameras[index]


def load_scene(path, alpha_blend=False):
    """`alpha_blend`: a file WITHOUT a blend section whose material descriptions ask for fractional opacity (material_blend_from_description) gets a blend table
    from them, and such a UsdPreviewSurface is PBR, not glass.  Off (the default): the translations of before.  A file's own blend section is always honoured."""
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != MAGIC:
        raise ValueError(f"{path}: not a .skscene file")
    version, nsec = struct.unpack_from("<II", blob, 8)
    if version != VERSION:
        raise ValueError(f"{path}: version {version}, this reader knows {VERSION}")
    known = {tag: (key, dt) for tag, key, dt in _SECTIONS}
    arrays = {key: np.zeros((0,) + dt.shape, dt.base if dt.shape else dt) for _, key, dt in _SECTIONS}
    cameras, descs = [], None
    tex_desc, texels = np.zeros(0, S.TEXTURE_DESC), np.zeros(0, np.uint32)
    blend = shapes = None
    off = 16
    for _ in range(nsec):
        if off + 16 > len(blob):
            raise ValueError(f"{path}: truncated section header")
        tag = blob[off:off + 4]
        esz, cnt = struct.unpack_from("<IQ", blob, off + 4)
        off += 16
        nbytes = esz * cnt
        if off + nbytes > len(blob):
            raise ValueError(f"{path}: section {tag!r} runs past the end of the file")
        data = blob[off:off + nbytes]
        off += nbytes + (-nbytes % 8)
        if tag in known:
            key, dt = known[tag]
            if esz != dt.itemsize:
                raise ValueError(f"{path}: section {tag!r} has {esz}-byte elements, expected {dt.itemsize}")
            a = np.frombuffer(data, dtype=dt.base if dt.shape else dt).copy()
            arrays[key] = a.reshape((-1,) + dt.shape) if dt.shape else a
        elif tag == b"CAMR":
            for rec in np.frombuffer(data, dtype=CAMERA):
                cameras.append(LoadedCamera(rec["view"], float(rec["fov"]), float(rec["znear"]), float(rec["zfar"])))
        elif tag == b"MDSC":
            descs = json.loads(bytes(data).decode())
        elif tag == b"TXDS" and esz == S.TEXTURE_DESC.itemsize:
            tex_desc = np.frombuffer(data, dtype=S.TEXTURE_DESC).copy()
        elif tag == b"MBLD" and esz == S.MATERIAL_BLEND.itemsize:
            blend = np.frombuffer(data, dtype=S.MATERIAL_BLEND).copy()
        elif tag == b"LSHP" and esz == S.LIGHT_SHAPE.itemsize:
            shapes = np.frombuffer(data, dtype=S.LIGHT_SHAPE).copy()
        elif tag == b"TXEL" and esz == 4:
            texels = np.frombuffer(data, dtype=np.uint32).copy()
        # unknown tags: skipped
    arrays["textures"] = []
    for k, d in enumerate(tex_desc):
        n = int(d["width"]) * int(d["height"])
        if n == 0 or int(d["offset"]) + n > len(texels):
            raise ValueError(f"{path}: texture {k} reaches outside the texel section")
        arrays["textures"].append(texels[int(d["offset"]):int(d["offset"]) + n].view(np.uint8).reshape(int(d["height"]), int(d["width"]), 4).copy())
    if len(arrays["materials"]) == 0:
        arrays["materials"] = materials_from_descriptions(descs or [], alpha_blend and blend is None)
        em = emission_from_descriptions(descs or [])  # (the format is unchanged: emission travels as material parameters)
        if em is not None:
            arrays["emission"] = em
    mt = material_textures_from_descriptions(descs or [])  # (likewise; the parameters name TXDS entries, 1-based -- with or without MATL, which has no room for them)
    if mt is not None and len(mt) <= len(arrays["materials"]):
        arrays["material_textures"] = mt
    ct = material_cutouts_from_descriptions(descs or [])  # (likewise)
    if ct is not None and len(ct) <= len(arrays["materials"]):
        arrays["material_cutouts"] = ct
    if blend is None and alpha_blend:
        blend = material_blends_from_descriptions(descs or [])
    if blend is not None and len(blend) <= len(arrays["materials"]):
        arrays["material_blend"] = blend
    if shapes is not None and len(shapes) <= len(arrays["lights"]):
        arrays["light_shapes"] = shapes
    if not cameras:
        cameras.append(S.Camera())
    validate(arrays)
    return LoadedScene(arrays, cameras, descs)


def validate(arrays):
    """The range checks the reference never makes (it trusts its own loaders); a dump comes from outside."""
    nv, ni = len(arrays["vertices"]), len(arrays["indices"])
    for k, m in enumerate(arrays["meshes"]):
        if int(m["index_offset"]) + int(m["index_count"]) > ni or int(m["vertex_offset"]) + int(m["vertex_count"]) > nv:
            raise ValueError(f"mesh {k} reaches outside the index / vertex buffers")
        if m["index_count"] % 3:
            raise ValueError(f"mesh {k}: index count {m['index_count']} is not a multiple of 3")
    nm, nc, nl = len(arrays["meshes"]), len(arrays["curves"]), len(arrays["lights"])
    for k, i in enumerate(arrays["instances"]):
        t, g = int(i["type"]), int(i["geom_id"])
        if t not in (S.INSTANCE_MESH, S.INSTANCE_LIGHT, S.INSTANCE_CURVE):
            raise ValueError(f"instance {k}: unknown type {t}")
        if (t == S.INSTANCE_CURVE and g >= nc) or (t != S.INSTANCE_CURVE and g >= nm):
            raise ValueError(f"instance {k}: geometry {g} does not exist")
        if t == S.INSTANCE_LIGHT and int(i["light_id"]) >= nl:
            raise ValueError(f"instance {k}: light {int(i['light_id'])} does not exist")
    npts, nw, nvc = len(arrays["curve_points"]), len(arrays["curve_radii"]), len(arrays["curve_vertex_counts"])
    nt = len(arrays.get("textures") or [])
    for k, m in enumerate(arrays["materials"]):
        if int(m["base_color_texture"]) > nt or int(m["normal_texture"]) > nt:
            raise ValueError(f"material {k} refers to a texture that does not exist")
    for k, e in enumerate(arrays.get("material_textures", [])):
        if max(int(e["roughness_texture"]), int(e["metallic_texture"]), int(e["emission_texture"])) > nt:
            raise ValueError(f"material {k}: a roughness / metallic / emission map refers to a texture that does not exist")
    for k, e in enumerate(arrays.get("material_cutouts", [])):
        if int(e["opacity_texture"]) > nt:
            raise ValueError(f"material {k}: the opacity map refers to a texture that does not exist")
    for k, e in enumerate(arrays.get("material_blend", [])):
        if int(e["opacity_texture"]) > nt:
            raise ValueError(f"material {k}: the blend entry's opacity map refers to a texture that does not exist")
    for k, c in enumerate(arrays["curves"]):
        if (int(c["points_start"]) + int(c["points_count"]) > npts or int(c["widths_start"]) + int(c["widths_count"]) > nw or
                int(c["vertex_counts_start"]) + int(c["vertex_counts_count"]) > nvc):
            raise ValueError(f"curve set {k} reaches outside the control-point / radius / count buffers")


# ---- MaterialDescription -> skh_material (what the HipRender adapter does inside Strelka: INTEGRATION.md section 1) ----
def _param(desc, name, default=None):
    for p in desc.get("params", []):
        if p.get("name") == name:
            return p.get("value", default)
    return default


def material_from_description(desc, alpha_blend=False):
    """`alpha_blend`: a UsdPreviewSurface whose opacity is a blend entry's (material_blend_from_description) is PBR, not glass.
    One reference MaterialDescription {file, name, params[{name, type, value}]} -> one MATERIAL record.
    default.mdl::default_material.diffuse_color (OptixRender.cpp:1090-1097, RenderPass.cpp:222-245) -> diffuse;
    OmniPBR.{diffuse_color_constant, reflection_roughness_constant, metallic_constant} (gltfloader.cpp:304-352) -> PBR;
    OmniGlass (gltfloader.cpp:354-406: enable_opacity, thin_walled, frosting_roughness; glass_ior when present) -> glass;
    UsdPreviewSurface parameter sets (HdStrelka's eMaterialX descriptions) -> PBR / glass; names containing "hair" -> the hair
    BSDF slot.  Unknown materials fall back to the default diffuse 0.8 grey."""
    m = np.zeros(1, S.MATERIAL)[0]
    m["base_color"], m["roughness"], m["specular"], m["ior"] = 0.8, 0.5, 0.5, 1.5
    name = (desc.get("name") or "") + " " + (desc.get("file") or "")
    low = name.lower()
    pnames = {p.get("name") for p in desc.get("params", [])}
    if pnames & {"diffuseColor", "useSpecularWorkflow", "specularColor", "clearcoat", "emissiveColor"}:
        # UsdPreviewSurface: HdStrelkaMaterial copies the node's parameters under their USD names (Material.cpp:52-150) and hands
        # the network to MaterialX -> MDL (RenderPass.cpp:164-172, type eMaterialX).  Spec defaults: diffuseColor 0.18,
        # roughness 0.5, metallic 0, ior 1.5, opacity 1; an opacity below 0.5 is treated as glass.
        # With an opacityThreshold > 0 the opacity is a CUTOUT's (material_cutout_from_description), never glass.
        opacity = float(_param(desc, "opacity", 1.0))
        m["type"] = S.MAT_GLASS if opacity < 0.5 and not float(_param(desc, "opacityThreshold", 0.0)) > 0.0 and not alpha_blend else S.MAT_PBR
        m["base_color"] = _param(desc, "diffuseColor", (0.18, 0.18, 0.18))
        m["roughness"] = float(_param(desc, "roughness", 0.5))
        m["metallic"] = float(_param(desc, "metallic", 0.0))
        m["ior"] = float(_param(desc, "ior", 1.5))
    elif "omniglass" in low or "glass" in low:
        m["type"] = S.MAT_GLASS
        m["base_color"] = _param(desc, "glass_color", (1.0, 1.0, 1.0))
        m["roughness"] = float(_param(desc, "frosting_roughness", 0.0))
        m["ior"] = float(_param(desc, "glass_ior", 1.491))  # OmniGlass.mdl default
    elif "omnipbr" in low or "pbr" in low:
        m["type"] = S.MAT_PBR
        m["base_color"] = _param(desc, "diffuse_color_constant", (0.2, 0.2, 0.2))  # OmniPBR.mdl default
        m["roughness"] = float(_param(desc, "reflection_roughness_constant", 0.5))
        m["metallic"] = float(_param(desc, "metallic_constant", 0.0))
    elif "hair" in low:
        # a hair material = df::chiang_hair_bsdf behind the `hair` slot (mdlPtxCodeGen.cpp:143-155); parameter names as in the
        # MDL specification of that distribution function, colour -> absorption by Chiang et al. 2016 eq. 9 when no
        # absorption_coefficient is given
        m["type"] = S.MAT_HAIR
        rn = float(_param(desc, "roughness_azimuthal", _param(desc, "roughness", 0.3)))
        sig = _param(desc, "absorption_coefficient", None)
        if sig is None:
            sig = S.hair_sigma_a_from_color(_param(desc, "diffuse_color", _param(desc, "color", (0.35, 0.2, 0.1))), rn)
        m["base_color"] = _param(desc, "diffuse_reflection_tint", (1.0, 1.0, 1.0))
        m["roughness"] = float(_param(desc, "roughness_R", _param(desc, "roughness", 0.3)))
        m["metallic"] = float(_param(desc, "roughness_TT", 0.0))
        m["specular"] = float(_param(desc, "roughness_TRT", 0.0))
        m["ior"] = float(_param(desc, "ior", 1.55))
        m["reserved"] = (sig[0], sig[1], sig[2], rn, float(_param(desc, "cuticle_angle", 0.035)), float(_param(desc, "diffuse_reflection_weight", 0.0)))
    else:
        m["type"] = S.MAT_DIFFUSE
        m["base_color"] = _param(desc, "diffuse_color", (0.8, 0.8, 0.8))
    return m


def emission_from_description(desc):
    """The radiance Le (linear RGB, three floats) the description's surfaces emit -- skh_set_emission's entry for the material; (0, 0, 0) = none.
    UsdPreviewSurface: emissiveColor.  OmniPBR: enable_emission ? emissive_color * emissive_intensity : 0 (the defaults of absent parameters: the
    white colour and intensity 1 a glTF factor is written with here, strelka_amd/gltf.py).  Other materials do not emit."""
    low = ((desc.get("name") or "") + " " + (desc.get("file") or "")).lower()
    pnames = {p.get("name") for p in desc.get("params", [])}
    if pnames & {"diffuseColor", "useSpecularWorkflow", "specularColor", "clearcoat", "emissiveColor"}:
        e = np.asarray(_param(desc, "emissiveColor", (0.0, 0.0, 0.0)), np.float32)
    elif "glass" not in low and "pbr" in low and _param(desc, "enable_emission", False):
        e = np.asarray(_param(desc, "emissive_color", (1.0, 1.0, 1.0)), np.float32) * np.float32(_param(desc, "emissive_intensity", 1.0))
    else:
        e = np.zeros(3, np.float32)
    return np.maximum(e.reshape(3), np.float32(0.0))  # (a negative value does not emit)


def emission_from_descriptions(descs):
    """(n, 3) float32 for skh_set_emission, or None when no description emits"""
    em = np.zeros((max(1, len(descs)), 3), np.float32)
    for k, d in enumerate(descs):
        em[k] = emission_from_description(d)
    return em if em.any() else None


def _texture_id(desc, name, texture_ids=None):
    """a texture parameter's value: the 1-based id into the scene's texture list, or a uri that `texture_ids` maps to one; anything else = none"""
    v = _param(desc, name, 0)
    if isinstance(v, str):
        return int((texture_ids or {}).get(v, 0))
    return int(v) if isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 else 0


def _is_omnipbr(desc):
    low = ((desc.get("name") or "") + " " + (desc.get("file") or "")).lower()
    pnames = {p.get("name") for p in desc.get("params", [])}
    if pnames & {"diffuseColor", "useSpecularWorkflow", "specularColor", "clearcoat", "emissiveColor"}:
        return False
    return "glass" not in low and "pbr" in low  # (material_from_description's OmniPBR branch)


def _mix_affine(constant, influence):
    """OmniPBR's mix(constant, texel, influence) = constant (1 - influence) + texel influence as scale * texel + bias, in float32:
    scale = influence, bias = fl(constant * fl(1 - influence))"""
    w = np.float32(influence)
    return w, np.float32(np.float32(constant) * np.float32(np.float32(1.0) - w))


def material_textures_from_description(desc, texture_ids=None):
    """One MaterialDescription -> one S.MATERIAL_TEXTURES record (skh_set_material_textures' entry).  OmniPBR only; a texture parameter carries a 1-based
    texture id, or a uri that `texture_ids` (uri -> id, the glTF loader's) resolves; an unresolved one binds nothing.
      reflectionroughness_texture + reflection_roughness_texture_influence (default 0, OmniPBR.mdl) -> the roughness slot, channel r,
          scale = influence, bias = reflection_roughness_constant * (1 - influence); an influence of 0 binds nothing (the map has no say)
      metallic_texture + metallic_texture_influence -> the metallic slot, likewise
      enable_ORM_texture + ORM_texture -> roughness = g, metallic = b of ONE texture, both influences 1; r (occlusion) is ignored: the
          renderer has no ambient term it could scale.  Optional ORM_roughness_scale / ORM_metallic_scale (default 1; glTF's
          roughnessFactor / metallicFactor, strelka_amd/gltf.py) multiply the texel.  ORM wins over the standalone maps, as in OmniPBR.
      emissive_color_texture -> emission, rgb;  emissive_mask_texture -> emission, channel r, only without a colour texture
          (both only with enable_emission: emission_from_description gives the Le they scale)
    A standalone roughness / metallic map is read through channel r: an 8-bit grey image decodes to r = g = b here, so grey maps give
    MDL's value; for a coloured map MDL's mono look-up averages the three channels and this does not."""
    e = np.zeros(1, S.MATERIAL_TEXTURES)[0]
    e["emission_channel"] = S.EMISSION_RGB
    e["roughness_scale"] = e["metallic_scale"] = 1.0
    if not _is_omnipbr(desc):
        return e
    orm = _texture_id(desc, "ORM_texture", texture_ids) if _param(desc, "enable_ORM_texture", False) else 0
    if orm:
        e["roughness_texture"] = e["metallic_texture"] = orm
        e["roughness_channel"], e["metallic_channel"] = 1, 2
        e["roughness_scale"] = np.float32(_param(desc, "ORM_roughness_scale", 1.0))
        e["metallic_scale"] = np.float32(_param(desc, "ORM_metallic_scale", 1.0))
    else:
        for slot, tex, infl, const, cdef in (("roughness", "reflectionroughness_texture", "reflection_roughness_texture_influence", "reflection_roughness_constant", 0.5),
                                             ("metallic", "metallic_texture", "metallic_texture_influence", "metallic_constant", 0.0)):
            t, w = _texture_id(desc, tex, texture_ids), float(_param(desc, infl, 0.0))
            if t and w != 0.0:
                e[slot + "_texture"] = t
                e[slot + "_scale"], e[slot + "_bias"] = _mix_affine(float(_param(desc, const, cdef)), w)
    if _param(desc, "enable_emission", False):
        col, mask = _texture_id(desc, "emissive_color_texture", texture_ids), _texture_id(desc, "emissive_mask_texture", texture_ids)
        if col:
            e["emission_texture"], e["emission_channel"] = col, S.EMISSION_RGB
        elif mask:
            e["emission_texture"], e["emission_channel"] = mask, 0
    return e


def material_textures_from_descriptions(descs, texture_ids=None):
    """S.MATERIAL_TEXTURES array for skh_set_material_textures, or None when no description binds a map"""
    out = np.zeros(max(1, len(descs)), S.MATERIAL_TEXTURES)
    out["emission_channel"] = S.EMISSION_RGB
    out["roughness_scale"] = out["metallic_scale"] = 1.0
    for k, d in enumerate(descs):
        out[k] = material_textures_from_description(d, texture_ids)
    any_bound = (out["roughness_texture"] | out["metallic_texture"] | out["emission_texture"]).any()
    return out if any_bound else None


def material_cutout_from_description(desc, texture_ids=None):
    """One MaterialDescription -> one S.MATERIAL_CUTOUT record (skh_set_material_cutouts' entry); threshold 0 = the material is no cutout.
      OmniPBR, enable_opacity and opacity_threshold > 0: threshold = opacity_threshold.  With enable_opacity_texture and an opacity_texture that resolves:
          that texture, channel a for opacity_mode 0 (mono_alpha), else r -- a simplification: MDL's mono_average / mono_luminance / mono_maximum modes
          read a grey map's r = g = b identically and differ for coloured ones --, scale = the optional opacity_scale (default 1; glTF's baseColorFactor[3],
          strelka_amd/gltf.py), bias 0.  Without a texture: no look-up (texel = 1), scale 0, bias = opacity_constant (default 1, OmniPBR.mdl).
      UsdPreviewSurface, opacityThreshold > 0: no texture, scale 0, bias = opacity (default 1), threshold = opacityThreshold.
    Thresholds above 1 are clamped to 1."""
    e = np.zeros(1, S.MATERIAL_CUTOUT)[0]
    e["opacity_channel"], e["opacity_scale"] = 3, 1.0
    pnames = {p.get("name") for p in desc.get("params", [])}
    if pnames & {"diffuseColor", "useSpecularWorkflow", "specularColor", "clearcoat", "emissiveColor"}:
        th = float(_param(desc, "opacityThreshold", 0.0))
        if th > 0.0:
            e["opacity_scale"], e["opacity_bias"], e["threshold"] = 0.0, np.float32(_param(desc, "opacity", 1.0)), min(th, 1.0)
        return e
    if not _is_omnipbr(desc) or not _param(desc, "enable_opacity", False):
        return e
    th = float(_param(desc, "opacity_threshold", 0.0))
    if not th > 0.0:
        return e
    e["threshold"] = min(th, 1.0)
    t = _texture_id(desc, "opacity_texture", texture_ids) if _param(desc, "enable_opacity_texture", False) else 0
    if t:
        e["opacity_texture"], e["opacity_channel"] = t, 3 if int(_param(desc, "opacity_mode", 0)) == 0 else 0
        e["opacity_scale"] = np.float32(_param(desc, "opacity_scale", 1.0))
    else:
        e["opacity_scale"], e["opacity_bias"] = 0.0, np.float32(_param(desc, "opacity_constant", 1.0))
    return e


def material_cutouts_from_descriptions(descs, texture_ids=None):
    """S.MATERIAL_CUTOUT array for skh_set_material_cutouts, or None when no description is a cutout"""
    out = np.zeros(max(1, len(descs)), S.MATERIAL_CUTOUT)
    out["opacity_channel"], out["opacity_scale"] = 3, 1.0
    for k, d in enumerate(descs):
        out[k] = material_cutout_from_description(d, texture_ids)
    return out if (out["threshold"] > 0).any() else None


def material_blend_from_description(desc, texture_ids=None):
    """One MaterialDescription -> one S.MATERIAL_BLEND record (skh_set_material_blend's entry); active 0 = the material is not blended.  The cases
    material_cutout_from_description leaves: an opacity WITHOUT a threshold.
      OmniPBR, enable_opacity and no opacity_threshold > 0: with enable_opacity_texture and an opacity_texture that resolves: that texture, channel a for
          opacity_mode 0, else r, scale = the optional opacity_scale (default 1), bias 0.  Without a texture: scale 0, bias = opacity_constant (default 1) --
          and inactive when that constant is 1 or more (opaque either way).
      UsdPreviewSurface, opacity < 1 and no opacityThreshold > 0: no texture, scale 0, bias = opacity."""
    e = np.zeros(1, S.MATERIAL_BLEND)[0]
    e["opacity_channel"], e["opacity_scale"] = 3, 1.0
    pnames = {p.get("name") for p in desc.get("params", [])}
    if pnames & {"diffuseColor", "useSpecularWorkflow", "specularColor", "clearcoat", "emissiveColor"}:
        opacity = float(_param(desc, "opacity", 1.0))
        if opacity < 1.0 and not float(_param(desc, "opacityThreshold", 0.0)) > 0.0:
            e["opacity_scale"], e["opacity_bias"], e["active"] = 0.0, np.float32(opacity), 1
        return e
    if not _is_omnipbr(desc) or not _param(desc, "enable_opacity", False) or float(_param(desc, "opacity_threshold", 0.0)) > 0.0:
        return e
    t = _texture_id(desc, "opacity_texture", texture_ids) if _param(desc, "enable_opacity_texture", False) else 0
    if t:
        e["opacity_texture"], e["opacity_channel"] = t, 3 if int(_param(desc, "opacity_mode", 0)) == 0 else 0
        e["opacity_scale"], e["active"] = np.float32(_param(desc, "opacity_scale", 1.0)), 1
    else:
        const = float(_param(desc, "opacity_constant", 1.0))
        if const < 1.0:
            e["opacity_scale"], e["opacity_bias"], e["active"] = 0.0, np.float32(const), 1
    return e


def material_blends_from_descriptions(descs, texture_ids=None):
    """S.MATERIAL_BLEND array for skh_set_material_blend, or None when no description is blended"""
    out = np.zeros(max(1, len(descs)), S.MATERIAL_BLEND)
    out["opacity_channel"], out["opacity_scale"] = 3, 1.0
    for k, d in enumerate(descs):
        out[k] = material_blend_from_description(d, texture_ids)
    return out if out["active"].any() else None


def materials_from_descriptions(descs, alpha_blend=False):
    out = np.zeros(max(1, len(descs)), S.MATERIAL)
    if not descs:
        out[0]["base_color"] = 0.8  # material 0 = default.mdl::default_material
    for k, d in enumerate(descs):
        out[k] = material_from_description(d, alpha_blend)
    return out
