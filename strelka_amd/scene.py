"""Host-side mirror of the reference's scene model (``oka::Scene``, include/scene/scene.h, src/scene/scene.cpp).

Same names and argument meaning as the reference's C++ API (createMesh / createInstance / createCurve /
createLight / addMaterial / addCamera), producing the flat arrays the renderer uploads verbatim
(SURVEY.md section 8b "Inputs read from oka::Scene") in the C-ABI layouts of include/strelka_hip.h.
numpy only -- no GPU work happens here.
"""
import math

import numpy as np

# ---- C-ABI record layouts (include/strelka_hip.h) -------------------------------------------------------
VERTEX = np.dtype([("pos", np.float32, 3), ("tangent", np.uint32), ("normal", np.uint32), ("uv", np.uint32),
                   ("pad0", np.float32), ("pad1", np.float32)])  # scene.h:80-89, 32 B
MESH = np.dtype([("index_offset", np.uint32), ("index_count", np.uint32), ("vertex_offset", np.uint32),
                 ("vertex_count", np.uint32)])  # scene.h:21-27
CURVE = np.dtype([("vertex_counts_start", np.uint32), ("vertex_counts_count", np.uint32), ("points_start", np.uint32),
                  ("points_count", np.uint32), ("widths_start", np.uint32), ("widths_count", np.uint32)])  # scene.h:29-42
INSTANCE = np.dtype([("transform", np.float32, 12), ("type", np.uint32), ("geom_id", np.uint32),
                     ("material_id", np.uint32), ("light_id", np.uint32)])  # scene.h:44-60, 64 B
LIGHT = np.dtype([("points", np.float32, (4, 4)), ("color", np.float32, 4), ("normal", np.float32, 4),
                  ("type", np.int32), ("half_angle", np.float32), ("pad0", np.float32), ("pad1", np.float32)])  # 112 B
MATERIAL = np.dtype([("type", np.uint32), ("base_color", np.float32, 3), ("roughness", np.float32),
                     ("metallic", np.float32), ("specular", np.float32), ("ior", np.float32),
                     ("base_color_texture", np.uint32), ("normal_texture", np.uint32),  # texture ids: 1-based, 0 = none
                     ("reserved", np.float32, 6)])  # 64 B
MATERIAL_TEXTURES = np.dtype([("roughness_texture", np.uint32), ("metallic_texture", np.uint32), ("emission_texture", np.uint32),
                              ("roughness_channel", np.uint32), ("metallic_channel", np.uint32), ("emission_channel", np.uint32),
                              ("roughness_scale", np.float32), ("roughness_bias", np.float32), ("metallic_scale", np.float32),
                              ("metallic_bias", np.float32), ("reserved", np.uint32, 2)])  # skh_material_textures, 48 B
MATERIAL_CUTOUT = np.dtype([("opacity_texture", np.uint32), ("opacity_channel", np.uint32), ("opacity_scale", np.float32), ("opacity_bias", np.float32),
                            ("threshold", np.float32), ("reserved", np.uint32, 3)])  # skh_material_cutout, 32 B
EMISSION_RGB = 4  # emission_channel: the texel's rgb (0..3: that channel for all three)
TEXTURE_DESC = np.dtype([("offset", np.uint32), ("width", np.uint32), ("height", np.uint32), ("pad", np.uint32)])
FRAME_PARAMS = np.dtype([("view_to_world", np.float32, 16), ("clip_to_view", np.float32, 16),
                         ("subframe_index", np.uint32), ("samples_this_launch", np.uint32), ("spp_total", np.uint32),
                         ("max_depth", np.uint32), ("rect_light_sampling_method", np.uint32),
                         ("exposure", np.float32, 3), ("enable_accumulation", np.uint32), ("debug", np.uint32),
                         ("shadow_ray_tmin", np.float32), ("material_ray_tmin", np.float32)])  # 176 B
RAY = np.dtype([("origin", np.float32, 3), ("tmin", np.float32), ("dir", np.float32, 3), ("tmax", np.float32)])
HIT = np.dtype([("t", np.float32), ("instance_id", np.uint32), ("prim_id", np.uint32), ("u", np.float32),
                ("v", np.float32)])
assert VERTEX.itemsize == 32 and INSTANCE.itemsize == 64 and LIGHT.itemsize == 112
assert MATERIAL_TEXTURES.itemsize == 48 and MATERIAL_CUTOUT.itemsize == 32
MATERIAL_BLEND = np.dtype([("opacity_texture", np.uint32), ("opacity_channel", np.uint32), ("opacity_scale", np.float32), ("opacity_bias", np.float32),
                           ("active", np.uint32), ("reserved", np.uint32, 3)])  # skh_material_blend, 32 B
assert MATERIAL_BLEND.itemsize == 32
LIGHT_SHAPE = np.dtype([("flags", np.uint32), ("cos_outer", np.float32), ("cos_inner", np.float32), ("focus", np.float32), ("axis", np.float32, 3),
                        ("reserved", np.uint32)])  # skh_light_shape, 32 B
assert LIGHT_SHAPE.itemsize == 32
LIGHT_SHAPE_SAMPLE_DISC, LIGHT_SHAPE_CONE = 1, 2
assert MATERIAL.itemsize == 64 and FRAME_PARAMS.itemsize == 176 and RAY.itemsize == 32 and HIT.itemsize == 20
AOV_PARAMS = np.dtype([("view_to_world", np.float32, 16), ("clip_to_view", np.float32, 16), ("world_to_clip", np.float32, 16),
                       ("x0", np.uint32), ("y0", np.uint32), ("width", np.uint32), ("height", np.uint32), ("sample_index", np.uint32),
                       ("spp_total", np.uint32), ("tmin", np.float32), ("reserved", np.uint32, 5)])  # skh_aov_params, 240 B
assert AOV_PARAMS.itemsize == 240
AOV_PLANES = ("ids", "hit", "normal", "position", "geom_normal", "albedo", "texcoord")  # SKH_AOV_*: plane k's name
AOV_PIXEL_CENTRE = 0xFFFFFFFF

INSTANCE_MESH, INSTANCE_LIGHT, INSTANCE_CURVE = 0, 1, 2  # oka::Instance::Type
MAT_DIFFUSE, MAT_PBR, MAT_GLASS, MAT_HAIR = 0, 1, 2, 3
NO_ID = 0xFFFFFFFF


def pack_normals(n):
    """packNormals (scene.cpp:111-117 == HdStrelka/RenderPass.cpp:53-59): 10-10-10 bits, fp32 arithmetic."""
    n = np.asarray(n, np.float32).reshape(-1, 3)
    q = ((n + np.float32(1.0)) / np.float32(2.0) * np.float32(511.99999)).astype(np.uint32)
    return (q[:, 0] + (q[:, 1] << np.uint32(10)) + (q[:, 2] << np.uint32(20))).astype(np.uint32)


def pack_uv(uv):
    """packUV (HdStrelka/RenderPass.cpp:61-67): 16-16 bits over [-10, 10]."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    q = ((uv + np.float32(10.0)) / np.float32(20.0) * np.float32(16383.99999)).astype(np.uint32)
    return (q[:, 0] + (q[:, 1] << np.uint32(16))).astype(np.uint32)


def translate(t):
    m = np.eye(4, dtype=np.float64)
    m[:3, 3] = t
    return m


def scale(s):
    return np.diag([s[0], s[1], s[2], 1.0]).astype(np.float64)


def rotate(axis, angle_rad):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    x, y, z = a
    r = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s, 0],
                  [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s, 0],
                  [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c), 0], [0, 0, 0, 1]], np.float64)
    return r


def quat_from_euler_deg(e):
    """glm::quat(glm::radians(eulerDegrees)) as used by Scene::getTransform(desc) (scene.h:331-343)."""
    ex, ey, ez = [math.radians(v) * 0.5 for v in e]
    cx, cy, cz = math.cos(ex), math.cos(ey), math.cos(ez)
    sx, sy, sz = math.sin(ex), math.sin(ey), math.sin(ez)
    w = cx * cy * cz + sx * sy * sz
    x = sx * cy * cz - cx * sy * sz
    y = cx * sy * cz + sx * cy * sz
    z = cx * cy * sz - sx * sy * cz
    return np.array([w, x, y, z], np.float64)


def quat_to_mat4(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 0],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 0],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), 0], [0, 0, 0, 1]], np.float64)


class Camera:
    """oka::Camera (include/scene/camera.h, src/scene/camera.cpp): first-person, view dir -Z, reverse-Z projection."""

    def __init__(self, position=(0, 0, 10), fov=45.0, znear=0.1, zfar=1000.0, name="Default camera"):
        self.name = name
        self.fov = float(fov)
        self.znear, self.zfar = float(znear), float(zfar)
        self.position = np.asarray(position, np.float64)
        self.rotation = np.eye(4, dtype=np.float64)  # rotM (world -> camera rotation)
        self.view = None
        self.inv_perspective = None
        self.updateViewMatrix()

    def lookAt(self, eye, target, up=(0, 1, 0)):
        eye, target, up = [np.asarray(v, np.float64) for v in (eye, target, up)]
        f = target - eye
        f /= np.linalg.norm(f)
        s = np.cross(f, up)
        s /= np.linalg.norm(s)
        u = np.cross(s, f)
        r = np.eye(4)
        r[0, :3], r[1, :3], r[2, :3] = s, u, -f
        self.rotation = r
        self.position = eye
        self.updateViewMatrix()

    def updateViewMatrix(self):  # camera.cpp:10-23 (firstperson: view = rotM * transM)
        self.view = self.rotation @ translate(-self.position)

    def updateAspectRatio(self, aspect):  # camera.cpp:125-131 + 61-118: hand-written reverse-Z inverse, fp32
        n, f = np.float32(self.zfar), np.float32(self.znear)  # swapped for reverse z
        focal = np.float32(1.0) / np.float32(math.tan(np.float32(np.float32(self.fov) * np.float32(0.017453292519943295)) / np.float32(2.0)))
        x = np.float32(focal / np.float32(aspect))
        y = focal
        A = np.float32(n / (f - n))
        B = np.float32(f * A)
        one = np.float32(1.0)
        self.inv_perspective = np.array([[one / x, 0, 0, 0], [0, one / y, 0, 0], [0, 0, 0, -1.0], [0, 0, one / B, A / B]],
                                        np.float32)

    def view_to_world_rowmajor(self):  # OptixRender.cpp:953: transpose(inverse(view)) of a column-major glm matrix
        return np.linalg.inv(self.view).astype(np.float32).reshape(16)

    def clip_to_view_rowmajor(self):  # OptixRender.cpp:954
        return self.inv_perspective.astype(np.float32).reshape(16)


class Scene:
    """oka::Scene: flat CPU arrays the renderer uploads verbatim (scene.h:199-216)."""

    def __init__(self):
        self.mVertices = []  # list of VERTEX arrays
        self.mIndices = []
        self.mMeshes = []
        self.mCurves = []
        self.mCurvePoints = []
        self.mCurveWidths = []
        self.mCurveVertexCounts = []
        self.mInstances = []
        self.mLights = []
        self.mLightDesc = []
        self.mMaterials = []
        self.mTextures = []
        self.mCameras = []
        self._nverts = 0
        self._nidx = 0
        self._npoints = 0
        self._nvc = 0
        self.mRectLightMeshId = -1
        self.mSphereLightMeshId = -1
        self.mDiskLightMeshId = -1

    # -- scene.cpp:15-49
    def createMesh(self, vb, ib):
        vb = np.ascontiguousarray(vb, dtype=VERTEX)
        ib = np.ascontiguousarray(ib, dtype=np.uint32).reshape(-1)
        mesh_id = len(self.mMeshes)
        self.mMeshes.append((self._nidx, len(ib), self._nverts, len(vb)))
        self.mIndices.append(ib)
        self.mVertices.append(vb)
        self._nidx += len(ib)
        self._nverts += len(vb)
        return mesh_id

    # -- scene.cpp:51-87
    def createInstance(self, type_, geomId, materialId, transform, lightId=NO_ID):
        t = np.asarray(transform, np.float64).reshape(4, 4)
        inst_id = len(self.mInstances)
        self.mInstances.append((t[:3, :].astype(np.float32).reshape(12), type_, geomId, materialId & 0xFFFFFFFF, lightId))
        return inst_id

    # -- scene.cpp:89-95.  `material` is a dict of the fixed-layout argument block (skh_material)
    def addMaterial(self, type=MAT_DIFFUSE, base_color=(0.8, 0.8, 0.8), roughness=None, metallic=0.0, specular=0.5, ior=1.5,
                    base_color_texture=0, normal_texture=0, reserved=(0.0,) * 6, emission=None,
                    roughness_texture=0, metallic_texture=0, emission_texture=0, roughness_channel=0, metallic_channel=0,
                    emission_channel=EMISSION_RGB, roughness_scale=1.0, roughness_bias=0.0, metallic_scale=1.0, metallic_bias=0.0,
                    opacity_texture=None, opacity_channel=3, opacity_scale=1.0, opacity_bias=0.0, opacity_threshold=0.0,
                    opacity_blend=False):
        """`opacity_blend` makes the material BLENDED (include/strelka_hip.h, skh_set_material_blend): fractional opacity a = clamp01(opacity_scale *
        texel[opacity_channel] + opacity_bias) from the same `opacity_*` arguments -- a radiance ray takes a hit with probability a, a shadow ray's light is
        scaled by 1 - a.  Not together with `opacity_threshold`, not on an emitting material.
        `opacity_threshold` > 0 makes the material a CUTOUT (include/strelka_hip.h, skh_set_material_cutouts): a hit on one of its mesh surfaces counts iff
        clamp01(opacity_scale * texel[opacity_channel] + opacity_bias) >= opacity_threshold; `opacity_texture` None or 0 = no texture (texel = 1).
        `roughness_texture` / `metallic_texture` (MAT_PBR): value = clamp01(scale * texel[channel] + bias); `emission_texture`: Le = emission * texel
        (rgb, or one channel for all three) -- texture ids as base_color_texture's (include/strelka_hip.h, skh_set_material_textures).
        `emission`: linear RGB radiance Le the material's mesh surfaces emit from their front side (None = none; include/strelka_hip.h, skh_set_emission).
        MAT_GLASS: `roughness` is OmniGlass' frosting_roughness (default 0 = clear glass: gltfloader.cpp:354-406 sets it from the
        file's roughnessFactor, OmniGlass.mdl's own default is clear).  Other types: default 0.5.  MAT_HAIR: use addHairMaterial."""
        if roughness is None:
            roughness = 0.0 if type == MAT_GLASS else 0.5
        self.mMaterials.append((type, tuple(base_color), roughness, metallic, specular, ior, base_color_texture, normal_texture,
                                tuple(reserved)))
        if emission is not None and any(float(v) != 0.0 for v in emission):
            e = tuple(float(v) for v in emission)
            if len(e) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in e):
                raise ValueError("emission must be three finite values >= 0")
            self.__dict__.setdefault("mEmission", {})[len(self.mMaterials) - 1] = e  # (kept beside the list: its tuples are the argument blocks)
        if roughness_texture or metallic_texture or emission_texture:
            self.__dict__.setdefault("mMaterialTextures", {})[len(self.mMaterials) - 1] = (
                int(roughness_texture), int(metallic_texture), int(emission_texture), int(roughness_channel), int(metallic_channel), int(emission_channel),
                float(roughness_scale), float(roughness_bias), float(metallic_scale), float(metallic_bias), (0, 0))
        if float(opacity_threshold) != 0.0:
            if not 0.0 < float(opacity_threshold) <= 1.0 or int(opacity_channel) not in (0, 1, 2, 3):
                raise ValueError("opacity_threshold must lie in (0, 1] and opacity_channel in 0..3")
            self.__dict__.setdefault("mMaterialCutouts", {})[len(self.mMaterials) - 1] = (
                int(opacity_texture or 0), int(opacity_channel), float(opacity_scale), float(opacity_bias), float(opacity_threshold), (0, 0, 0))
        if opacity_blend:
            if float(opacity_threshold) != 0.0:
                raise ValueError("a material is a cutout (opacity_threshold) or blended (opacity_blend), not both")
            if emission is not None and any(float(v) != 0.0 for v in emission):
                raise ValueError("a blended material (opacity_blend) cannot emit")
            if int(opacity_channel) not in (0, 1, 2, 3) or not (math.isfinite(float(opacity_scale)) and math.isfinite(float(opacity_bias))):
                raise ValueError("opacity_channel must lie in 0..3, opacity_scale and opacity_bias must be finite")
            self.__dict__.setdefault("mMaterialBlend", {})[len(self.mMaterials) - 1] = (
                int(opacity_texture or 0), int(opacity_channel), float(opacity_scale), float(opacity_bias), 1, (0, 0, 0))
        return len(self.mMaterials) - 1

    def addHairMaterial(self, color=(0.35, 0.2, 0.1), roughness_r=0.3, roughness_n=0.3, roughness_tt=0.0, roughness_trt=0.0,
                        cuticle_angle=math.radians(2.0), ior=1.55, absorption=None, diffuse_weight=0.0, diffuse_tint=(1.0, 1.0, 1.0),
                        emission=None):
        """The arguments of df::chiang_hair_bsdf in the fixed-layout block (include/strelka_hip.h, SKH_MAT_HAIR).  `color` is the
        fibre's multiple-scattering albedo; the absorption coefficient follows from it by Chiang et al. 2016, eq. 9 -- what a hair
        material's MDL code does in front of the distribution function -- unless `absorption` gives sigma_a directly."""
        if absorption is None:
            absorption = hair_sigma_a_from_color(color, roughness_n)
        return self.addMaterial(MAT_HAIR, diffuse_tint, roughness=roughness_r, metallic=roughness_tt, specular=roughness_trt, ior=ior,
                                reserved=(absorption[0], absorption[1], absorption[2], roughness_n, cuticle_angle, diffuse_weight), emission=emission)

    def addTexture(self, rgba8):
        """RGBA8 image, rows top to bottom as stbi_load returns them (OptixRender.cpp:1191-1264).  Returns the texture ID
        materials refer to (1-based; 0 = no texture, as MDL's invalid texture)."""
        t = np.ascontiguousarray(rgba8, np.uint8)
        assert t.ndim == 3 and t.shape[2] == 4 and t.shape[0] > 0 and t.shape[1] > 0
        self.mTextures.append(t)
        return len(self.mTextures)

    def addCamera(self, camera):
        self.mCameras.append(camera)
        return len(self.mCameras) - 1

    def getCamera(self, index=0):
        return self.mCameras[index]

    # -- createCurve (scene.h declaration :399-402; HdStrelka/BasisCurves.cpp:189-232 supplies phantom points + radii)
    def createCurve(self, vertexCounts, points, widths):
        vertexCounts = np.ascontiguousarray(vertexCounts, np.uint32)
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        widths = np.ascontiguousarray(widths, np.float32).reshape(-1)
        cid = len(self.mCurves)
        self.mCurves.append((self._nvc, len(vertexCounts), self._npoints, len(points), self._npoints, len(widths)))
        self.mCurveVertexCounts.append(vertexCounts)
        self.mCurvePoints.append(points)
        self.mCurveWidths.append(widths)
        self._nvc += len(vertexCounts)
        self._npoints += len(points)
        return cid

    # -- light proxy meshes: scene.cpp:119-250
    def _createRectLightMesh(self):
        if self.mRectLightMeshId != -1:
            return self.mRectLightMeshId
        vb = np.zeros(4, VERTEX)
        vb["pos"] = [(0.5, 0.5, 0), (-0.5, 0.5, 0), (-0.5, -0.5, 0), (0.5, -0.5, 0)]
        vb["normal"] = pack_normals([(0, 0, 1)] * 4)
        self.mRectLightMeshId = self.createMesh(vb, [0, 1, 2, 2, 3, 0])
        return self.mRectLightMeshId

    def _createSphereLightMesh(self):
        if self.mSphereLightMeshId != -1:
            return self.mSphereLightMeshId
        segments = rings = 16
        pos = []
        for i in range(rings + 1):
            theta = np.float32(i) * np.float32(math.pi) / np.float32(rings)
            st, ct = np.float32(math.sin(theta)), np.float32(math.cos(theta))
            for j in range(segments + 1):
                phi = np.float32(j) * np.float32(2.0) * np.float32(math.pi) / np.float32(segments)
                sp, cp = np.float32(math.sin(phi)), np.float32(math.cos(phi))
                pos.append((cp * st, ct, sp * st))
        vb = np.zeros(len(pos), VERTEX)
        vb["pos"] = pos
        vb["normal"] = pack_normals(pos)
        ib = []
        for i in range(rings):
            for j in range(segments):
                p0 = i * (segments + 1) + j
                p1, p2 = p0 + 1, (i + 1) * (segments + 1) + j
                p3 = p2 + 1
                ib += [p0, p1, p2, p2, p1, p3]
        self.mSphereLightMeshId = self.createMesh(vb, ib)
        return self.mSphereLightMeshId

    def _createDiscLightMesh(self):
        if self.mDiskLightMeshId != -1:
            return self.mDiskLightMeshId
        pos = [(0, 0, 0), (1, 0, 0)]
        ib = []
        step = np.float32(2.0 * math.pi / 16)
        angle = np.float32(0)
        for _ in range(16):
            ib += [0, len(pos) - 1]
            angle = np.float32(angle + step)
            pos.append((math.cos(angle), math.sin(angle), 0.0))
            ib.append(len(pos) - 1)
        vb = np.zeros(len(pos), VERTEX)
        vb["pos"] = pos
        vb["normal"] = pack_normals([(0, 0, 1)] * len(pos))
        self.mDiskLightMeshId = self.createMesh(vb, ib)
        return self.mDiskLightMeshId

    @staticmethod
    def _light_transform(desc):  # Scene::getTransform(desc) scene.h:331-343
        t = translate(desc.get("position", (0, 0, 0)))
        r = quat_to_mat4(quat_from_euler_deg(desc.get("orientation", (0, 0, 0))))
        s = scale((desc.get("width", 1.0), desc.get("height", 1.0), 1.0))
        return t @ r @ s

    # -- Scene::createLight + updateLight: scene.cpp:306-408.  desc keys follow UniformLightDesc (scene.h:157-180)
    def createLight(self, desc):
        light_id = len(self.mLights)
        typ = int(desc["type"])
        use_xform = bool(desc.get("useXform", "xform" in desc))
        xform = np.asarray(desc.get("xform", np.eye(4)), np.float64).reshape(4, 4)
        radius = float(desc.get("radius", 0.0))
        L = np.zeros((), LIGHT)
        L["color"] = 1.0
        if typ == 0:
            sm = scale((desc["width"], desc["height"], 1.0))
            lt = xform @ sm if use_xform else self._light_transform(desc)
            for k, c in enumerate([(0.5, 0.5, 0, 1), (-0.5, 0.5, 0, 1), (-0.5, -0.5, 0, 1), (0.5, -0.5, 0, 1)]):
                L["points"][k] = (lt @ np.array(c, np.float64)).astype(np.float32)
            L["type"] = 0
            mesh, sm_inst = self._createRectLightMesh(), sm
        elif typ == 1:
            sm = scale((radius, radius, radius))
            lt = xform @ sm if use_xform else self._light_transform(desc)
            L["points"][0] = (radius, 0, 0, 0)
            L["points"][1] = (lt @ np.array([0, 0, 0, 1.0])).astype(np.float32)
            L["points"][2] = (lt @ np.array([1.0, 0, 0, 0])).astype(np.float32)
            L["points"][3] = (lt @ np.array([0, 1.0, 0, 0])).astype(np.float32)
            L["normal"] = (lt @ np.array([0, 0, 1.0, 0])).astype(np.float32)
            L["type"] = 1
            mesh, sm_inst = self._createDiscLightMesh(), sm
        elif typ == 2:
            lt = xform if use_xform else self._light_transform(desc)
            L["points"][0] = (radius, 0, 0, 0)
            L["points"][1] = (lt @ np.array([0, 0, 0, 1.0])).astype(np.float32)
            L["type"] = 2
            mesh, sm_inst = self._createSphereLightMesh(), scale((radius, radius, radius))
        elif typ == 3:
            L["type"] = 3
            L["half_angle"] = desc["halfAngle"]
            lt = xform if use_xform else self._light_transform(desc)
            n = lt @ np.array([0, 0, -1.0, 0])
            L["normal"] = (n / np.linalg.norm(n)).astype(np.float32)
            # scene.cpp:337-345: a light instance of MESH 0 scaled by desc.radius (0 for distant lights):
            # degenerate and unhittable, kept for index parity with the reference
            mesh, sm_inst = 0, scale((radius, radius, radius))
        else:
            raise ValueError("unknown light type")
        col = np.asarray(desc.get("color", (1, 1, 1)), np.float32)
        L["color"] = np.append(col, np.float32(1.0)) * np.float32(desc.get("intensity", 1.0))
        self.mLights.append(L)
        self.mLightDesc.append(dict(desc))
        shape = self._light_shape(desc, typ, L, lt)
        if shape is not None:
            if not hasattr(self, "mLightShapes"):
                self.mLightShapes = {}
            self.mLightShapes[light_id] = shape
        transform = (xform @ sm_inst) if use_xform else self._light_transform(desc)
        self.createInstance(INSTANCE_LIGHT, mesh, NO_ID, transform, light_id)
        return light_id

    # -- light shapes: not in the reference's UniformLightDesc; what an HdStrelkaLight with a UsdLux ShapingAPI would hand over
    @staticmethod
    def _light_shape(desc, typ, L, lt):
        """the skh_light_shape of a light description, None without one.  Keys: "sample": True (disks: the light takes part in next-event estimation);
        "coneAngle" (radians, shaping:cone:angle), "coneSoftness" (0..1), "focus" (>= 0); "axis" (world space; default: the light's own emission normal for
        rect and disk lights, xform * (0, 0, -1) for a sphere light)."""
        sample, cone = bool(desc.get("sample", False)), "coneAngle" in desc
        if sample and typ != 1:
            raise ValueError('"sample" is for disk lights (type 1): the other types are sampled already')
        if cone and typ not in (0, 1, 2):
            raise ValueError("a shaping cone needs a rect, disk or sphere light")
        if not sample and not cone:
            return None
        e = np.zeros((), LIGHT_SHAPE)
        e["cos_outer"] = e["cos_inner"] = -1.0
        e["flags"] = (LIGHT_SHAPE_SAMPLE_DISC if sample else 0) | (LIGHT_SHAPE_CONE if cone else 0)
        if cone:
            angle, soft = float(desc["coneAngle"]), float(desc.get("coneSoftness", 0.0))
            if not (0.0 <= angle <= math.pi) or not (0.0 <= soft <= 1.0):
                raise ValueError("coneAngle must lie in [0, pi] and coneSoftness in [0, 1]")
            co, ci = np.float32(math.cos(angle)), np.float32(math.cos(angle * (1.0 - soft)))
            e["cos_outer"], e["cos_inner"] = co, max(co, ci)
            e["focus"] = float(desc.get("focus", 0.0))
            if "axis" in desc:
                a = np.asarray(desc["axis"], np.float64)
            elif typ == 0:  # calc_light_normal: -normalize(cross(p1 - p0, p3 - p0))
                p = L["points"].astype(np.float64)
                a = -np.cross(p[1, :3] - p[0, :3], p[3, :3] - p[0, :3])
            elif typ == 1:
                a = L["normal"][:3].astype(np.float64)
            else:
                a = (lt @ np.array([0, 0, -1.0, 0]))[:3]
            e["axis"] = (a / np.linalg.norm(a)).astype(np.float32) + np.float32(0.0)  # (+ 0: no negative zeros)
        return e

    # -- environment (dome) light: not in the reference's Scene; what an HdStrelkaLight of type domeLight would hand over
    def setEnvironment(self, rgb, scale=(1.0, 1.0, 1.0), world_to_env=None):
        """rgb: (H, W, 3) linear floats, lat-long, row 0 = the +Y pole, column 0 at phi = 0 on +X; None removes it"""
        if rgb is None:
            self.mEnvironment = None
            return
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("the environment map must be an (H, W, 3) array")
        m = np.eye(3, dtype=np.float32) if world_to_env is None else np.ascontiguousarray(world_to_env, np.float32).reshape(3, 3)
        self.mEnvironment = {"rgb": rgb, "scale": np.ascontiguousarray(scale, np.float32).reshape(3), "world_to_env": m}

    # -- flat getters (scene.h:229-327) in C-ABI layouts
    def arrays(self):
        def cat(lst, dtype, shape=None):
            if not lst:
                return np.zeros((0,) + (shape or ()), dtype)
            return np.ascontiguousarray(np.concatenate(lst), dtype=dtype)

        meshes = np.zeros(len(self.mMeshes), MESH)
        for i, m in enumerate(self.mMeshes):
            meshes[i] = m
        curves = np.zeros(len(self.mCurves), CURVE)
        for i, c in enumerate(self.mCurves):
            curves[i] = c
        inst = np.zeros(len(self.mInstances), INSTANCE)
        for i, (t, ty, g, m, l) in enumerate(self.mInstances):
            inst[i] = (t, ty, g, m, l)
        lights = np.zeros(len(self.mLights), LIGHT)
        for i, l in enumerate(self.mLights):
            lights[i] = l
        mats = np.zeros(max(1, len(self.mMaterials)), MATERIAL)
        if not self.mMaterials:  # material 0 = default.mdl::default_material (OptixRender.cpp:1090-1097)
            mats[0]["base_color"] = 0.8
        for i, (ty, bc, r, me, sp, ior, bt, nt, rsv) in enumerate(self.mMaterials):
            mats[i]["type"], mats[i]["base_color"], mats[i]["roughness"] = ty, bc, r
            mats[i]["metallic"], mats[i]["specular"], mats[i]["ior"] = me, sp, ior
            mats[i]["base_color_texture"], mats[i]["normal_texture"] = bt, nt
            mats[i]["reserved"] = rsv
        out = {
            "vertices": cat(self.mVertices, VERTEX),
            "indices": cat(self.mIndices, np.uint32),
            "meshes": meshes,
            "curves": curves,
            "curve_points": cat(self.mCurvePoints, np.float32, (3,)),
            "curve_radii": cat(self.mCurveWidths, np.float32),
            "curve_vertex_counts": cat(self.mCurveVertexCounts, np.uint32),
            "instances": inst,
            "lights": lights,
            "materials": mats,
            "textures": list(self.mTextures),
        }
        if getattr(self, "mEnvironment", None) is not None:  # (only then: a scene without one has the keys it always had)
            out["environment"] = self.mEnvironment
        if getattr(self, "mEmission", None):  # (likewise only when some material emits; the CPU oracle does not read it)
            em = np.zeros((len(mats), 3), np.float32)
            for i, e in self.mEmission.items():
                em[i] = e
            out["emission"] = em
        if getattr(self, "mMaterialTextures", None):  # (likewise only when some material binds one)
            mt = np.zeros(len(mats), MATERIAL_TEXTURES)
            mt["emission_channel"] = EMISSION_RGB
            mt["roughness_scale"] = mt["metallic_scale"] = 1.0
            for i, e in self.mMaterialTextures.items():
                mt[i] = e
            out["material_textures"] = mt
        if getattr(self, "mMaterialCutouts", None):  # (likewise only when some material is a cutout)
            ct = np.zeros(len(mats), MATERIAL_CUTOUT)
            ct["opacity_channel"], ct["opacity_scale"] = 3, 1.0
            for i, e in self.mMaterialCutouts.items():
                ct[i] = e
            out["material_cutouts"] = ct
        if getattr(self, "mMaterialBlend", None):  # (likewise only when some material is blended)
            bt = np.zeros(len(mats), MATERIAL_BLEND)
            bt["opacity_channel"], bt["opacity_scale"] = 3, 1.0
            for i, e in self.mMaterialBlend.items():
                bt[i] = e
            out["material_blend"] = bt
        if getattr(self, "mLightShapes", None):  # (likewise only when some light has a shape)
            ls = np.zeros(len(lights), LIGHT_SHAPE)
            ls["cos_outer"] = ls["cos_inner"] = -1.0
            for i, e in self.mLightShapes.items():
                ls[i] = e
            out["light_shapes"] = ls
        return out


def hair_sigma_a_from_color(color, roughness_n=0.3):
    """Absorption coefficient that gives a fibre the multiple-scattering albedo `color` at azimuthal roughness beta_n:
    Chiang et al. 2016, eq. 9 (pbrt-v3 HairBSDF::SigmaAFromReflectance)."""
    b = float(roughness_n)
    d = 5.969 - 0.215 * b + 2.532 * b ** 2 - 10.73 * b ** 3 + 5.574 * b ** 4 + 0.245 * b ** 5
    c = np.clip(np.asarray(color, np.float64), 1e-4, 1.0)
    return tuple(float(x) for x in (np.log(c) / d) ** 2)


def pack_textures(textures):
    """list of HxWx4 uint8 images -> (TEXTURE_DESC array, uint32 texel array) in the packed form the renderer keeps on the device"""
    desc = np.zeros(len(textures), TEXTURE_DESC)
    off, parts = 0, []
    for k, t in enumerate(textures):
        t = np.ascontiguousarray(t, np.uint8)
        desc[k] = (off, t.shape[1], t.shape[0], 0)
        parts.append(t.reshape(-1, 4).view(np.uint32).reshape(-1))
        off += t.shape[0] * t.shape[1]
    texels = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return desc, np.ascontiguousarray(texels, np.uint32)


def make_vertices(positions, normals=None, uvs=None, tangents=None):
    """Pack float attributes into the 32-byte Vertex the way HdStrelka's _BakeMeshInstance does
    (RenderPass.cpp:69-130): normal/tangent 10-10-10, uv 16-16 with V flipped by the caller."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    vb = np.zeros(len(positions), VERTEX)
    vb["pos"] = positions
    if normals is not None:
        vb["normal"] = pack_normals(normals)
    if tangents is not None:
        vb["tangent"] = pack_normals(tangents)
    if uvs is not None:
        vb["uv"] = pack_uv(uvs)
    return vb


def deindex(positions, tris):
    """HdStrelkaMesh::_UpdateGeometry (Mesh.cpp:123-179): 3 fresh vertices per triangle, flat face normals when no
    primvar is authored, tangent = cross(n, X|Y).  Returns (vertices, indices 0..3T-1)."""
    positions = np.asarray(positions, np.float32)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    p = positions[tris.reshape(-1)]
    p3 = p.reshape(-1, 3, 3).astype(np.float64)
    fn = np.cross(p3[:, 1] - p3[:, 0], p3[:, 2] - p3[:, 0])
    ln = np.linalg.norm(fn, axis=1, keepdims=True)
    fn = fn / np.where(ln > 0, ln, 1.0)
    n = np.repeat(fn, 3, axis=0)
    ax = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t = np.cross(n, ax)
    lt = np.linalg.norm(t, axis=1, keepdims=True)
    t = t / np.where(lt > 0, lt, 1.0)
    vb = make_vertices(p, n, None, t)
    return vb, np.arange(len(p), dtype=np.uint32)


def frame_params(camera, width, height, subframe_index=0, samples_this_launch=1, spp_total=64, max_depth=4,
                 rect_light_sampling_method=0, exposure=None, enable_accumulation=1, debug=0, shadow_ray_tmin=0.0,
                 material_ray_tmin=0.0):
    """The Params fields OptiXRender::render fills per call (OptixRender.cpp:936-1004)."""
    camera.updateAspectRatio(width / float(height))
    camera.updateViewMatrix()
    p = np.zeros((), FRAME_PARAMS)
    p["view_to_world"] = camera.view_to_world_rowmajor()
    p["clip_to_view"] = camera.clip_to_view_rowmajor()
    p["subframe_index"], p["samples_this_launch"], p["spp_total"] = subframe_index, samples_this_launch, spp_total
    p["max_depth"], p["rect_light_sampling_method"] = max_depth, rect_light_sampling_method
    p["exposure"] = default_exposure() if exposure is None else exposure
    p["enable_accumulation"], p["debug"] = enable_accumulation, debug
    p["shadow_ray_tmin"], p["material_ray_tmin"] = shadow_ray_tmin, material_ray_tmin
    return p


def aov_params(camera, width, height, region=None, sample_index=None, spp_total=64, tmin=0.0):
    """skh_aov_params for skh_render_aovs: the two matrices as frame_params fills them; world_to_clip = inverse(clip_to_view) . inverse(view_to_world) of
    those float32 matrices, in float64, rounded once.  `region` (x0, y0, width, height) or None = the whole image; `sample_index` None = the pixel centre."""
    f = frame_params(camera, width, height)
    p = np.zeros((), AOV_PARAMS)
    p["view_to_world"], p["clip_to_view"] = f["view_to_world"], f["clip_to_view"]
    v2w, c2v = (np.asarray(f[k], np.float64).reshape(4, 4) for k in ("view_to_world", "clip_to_view"))
    p["world_to_clip"] = (np.linalg.inv(c2v) @ np.linalg.inv(v2w)).astype(np.float32).reshape(16)
    if region is not None:
        p["x0"], p["y0"], p["width"], p["height"] = region
    p["sample_index"] = AOV_PIXEL_CENTRE if sample_index is None else sample_index
    p["spp_total"], p["tmin"] = spp_total, tmin
    return p


DENOISE_PARAMS = np.dtype([("width", np.uint32), ("height", np.uint32), ("first_level", np.uint32), ("levels", np.uint32), ("sigma_color", np.float32),
                           ("sigma_normal", np.float32), ("sigma_plane", np.float32), ("albedo_floor", np.float32), ("flags", np.uint32),
                           ("reserved", np.uint32, 7)])  # skh_denoise_params, 64 B
assert DENOISE_PARAMS.itemsize == 64
DENOISE_DEMODULATE, DENOISE_REMODULATE = 1, 2
DENOISE_MAX_LEVEL = 8
# the defaults of denoise_params (DESIGN.md section 2 "Denoiser" gives the reasons)
DENOISE_SIGMA_NORMAL = 0.3       # |N(q) - N(p)| at which the normal term is 1: 17 degrees between unit normals
DENOISE_PLANE_FRACTION = 0.005   # sigma_plane as a fraction of the scene's bounding-box diagonal
DENOISE_ALBEDO_FLOOR = 0.05


def scene_diagonal(arr):
    """length of the diagonal of the world-space bounding box of a scene's mesh instances (`arr`: Scene.arrays()); the box of each mesh's own box under its
    instance's transform, which contains the instance"""
    pos, boxes = arr["vertices"]["pos"], {}
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in arr["instances"]:
        if int(inst["type"]) != INSTANCE_MESH:
            continue
        g = int(inst["geom_id"])
        if g not in boxes:
            m = arr["meshes"][g]
            v = pos[int(m["vertex_offset"]):int(m["vertex_offset"]) + int(m["vertex_count"])].astype(np.float64)
            boxes[g] = None if len(v) == 0 else np.array([[x, y, z] for x in (v[:, 0].min(), v[:, 0].max()) for y in (v[:, 1].min(), v[:, 1].max())
                                                          for z in (v[:, 2].min(), v[:, 2].max())])
        if boxes[g] is None:
            continue
        t = np.asarray(inst["transform"], np.float64).reshape(3, 4)
        w = boxes[g] @ t[:, :3].T + t[:, 3]
        lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    if not np.isfinite(lo).all():
        raise ValueError("the scene has no mesh instance to take a bounding box from")
    return float(np.linalg.norm(hi - lo))


def denoise_sigma_color(image, guides=None, albedo_floor=DENOISE_ALBEDO_FLOOR, demodulate=True):
    """the default sigma_color for an (h, w, 4) image: DENOISE_COLOR_FACTOR x the mean, over the pixels the filter works on, of the mean channel of its first level's
    input -- with `guides` ({"ids", "albedo"}: render_guides') the surface pixels and the demodulated colour, without them every finite pixel of the image as it is"""
    c = np.asarray(image, np.float64)[..., :3]
    ok = np.isfinite(c).all(axis=-1)
    if guides is not None and guides.get("ids") is not None:
        kind = np.asarray(guides["ids"])[..., 3]
        ok &= (kind == 1) | (kind == 2)
    if demodulate and guides is not None and guides.get("albedo") is not None:
        a = np.asarray(guides["albedo"], np.float64)[..., :3]
        with np.errstate(all="ignore"):
            c = c / np.where(a > albedo_floor, a, albedo_floor)
    if not ok.any():
        return 1.0
    level = float(np.abs(c[ok]).mean())
    return DENOISE_COLOR_FACTOR * level if level > 0.0 and np.isfinite(level) else 1.0


DENOISE_COLOR_FACTOR = 2.0


def denoise_params(width, height, levels=5, sigma_color=None, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_plane=None, first_level=0, albedo_floor=DENOISE_ALBEDO_FLOOR,
                   demodulate=True, remodulate=True, image=None, guides=None, exposure=None, scene=None):
    """skh_denoise_params.  sigma_color applies to the first level's input (the demodulated colour when `demodulate`) and the filter halves it per level; None:
    denoise_sigma_color(`image`, `guides`) when the image to be filtered is given, else 1 / the mean exposure factor (`exposure`: frame_params'; None =
    default_exposure()) -- the radiance a Reinhard tonemap under that exposure shows as mid-grey, which is what a host that never sees the image can know of it.
    sigma_plane is in scene units; None: DENOISE_PLANE_FRACTION of scene_diagonal(`scene`) (`scene`: Scene.arrays())."""
    p = np.zeros((), DENOISE_PARAMS)
    p["width"], p["height"], p["first_level"], p["levels"] = width, height, first_level, levels
    if sigma_color is None and image is not None:
        sigma_color = denoise_sigma_color(image, guides, albedo_floor, demodulate)
    if sigma_color is None:
        e = np.asarray(default_exposure() if exposure is None else exposure, np.float64).reshape(-1)
        sigma_color = 1.0 / float(e.mean())
    if sigma_plane is None:
        if scene is None:
            raise ValueError("sigma_plane is in scene units: give it, or give `scene` to take it as a fraction of the bounding-box diagonal")
        sigma_plane = DENOISE_PLANE_FRACTION * scene_diagonal(scene)
    p["sigma_color"], p["sigma_normal"], p["sigma_plane"], p["albedo_floor"] = sigma_color, sigma_normal, sigma_plane, albedo_floor
    p["flags"] = (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_REMODULATE if remodulate else 0)
    return p


TEMPORAL_PARAMS = np.dtype([("width", np.uint32), ("height", np.uint32), ("prev_world_to_clip", np.float32, 16), ("normal_min", np.float32),
                            ("plane_tolerance", np.float32), ("max_history", np.float32), ("initial_length", np.float32), ("albedo_floor", np.float32),
                            ("flags", np.uint32), ("reserved", np.uint32, 8)])  # skh_temporal_params, 128 B
assert TEMPORAL_PARAMS.itemsize == 128
TEMPORAL_DEMODULATE = 1
# the defaults of temporal_params (DESIGN.md section 2 "Temporal accumulation" gives the reasons)
TEMPORAL_NORMAL_MIN = 0.9     # cos 26 degrees: the two pixel-centre normals of one smooth surface a camera move apart, not a crease
TEMPORAL_MAX_HISTORY = 32.0   # alpha never below 1/32


def temporal_params(width, height, prev_aov_params=None, normal_min=TEMPORAL_NORMAL_MIN, plane_tolerance=None, max_history=TEMPORAL_MAX_HISTORY, initial_length=1.0,
                    albedo_floor=DENOISE_ALBEDO_FLOOR, demodulate=True, scene=None):
    """skh_temporal_params.  `prev_aov_params` (aov_params' record the previous guide planes were rendered with) supplies prev_world_to_clip; None: the identity,
    for a call without a previous frame.  plane_tolerance is in scene units; None: DENOISE_PLANE_FRACTION of scene_diagonal(`scene`) (`scene`: Scene.arrays()),
    the denoiser's rule for its sigma_plane."""
    p = np.zeros((), TEMPORAL_PARAMS)
    p["width"], p["height"] = width, height
    p["prev_world_to_clip"] = np.eye(4, dtype=np.float32).reshape(16) if prev_aov_params is None else np.asarray(prev_aov_params["world_to_clip"], np.float32).reshape(16)
    if plane_tolerance is None:
        if scene is None:
            raise ValueError("plane_tolerance is in scene units: give it, or give `scene` to take it as a fraction of the bounding-box diagonal")
        plane_tolerance = DENOISE_PLANE_FRACTION * scene_diagonal(scene)
    p["normal_min"], p["plane_tolerance"], p["max_history"], p["initial_length"], p["albedo_floor"] = normal_min, plane_tolerance, max_history, initial_length, albedo_floor
    p["flags"] = TEMPORAL_DEMODULATE if demodulate else 0
    return p


INSTANCE_MOTION = np.dtype([("to_prev", np.float32, 12), ("normal_to_prev", np.float32, 9), ("flags", np.uint32), ("reserved", np.uint32, 2)])  # skh_instance_motion, 96 B
assert INSTANCE_MOTION.itemsize == 96
MOTION_MOVED, MOTION_DROP = 1, 2


def instance_motion(prev_instances, instances):
    """the skh_instance_motion table that takes the current frame's guide planes back to the previous frame: one entry per instance, derived from the two
    INSTANCE tables' transforms by the library's own skh_instance_motion_from_transforms (host only, no GPU).  An instance the previous table does not have
    (the current one is longer) gets MOVED | DROP: it has no history."""
    import ctypes as C

    from . import capi

    lib = capi.load()
    prev = np.ascontiguousarray(prev_instances, dtype=INSTANCE).reshape(-1)
    cur = np.ascontiguousarray(instances, dtype=INSTANCE).reshape(-1)
    table = np.zeros(len(cur), INSTANCE_MOTION)
    for i in range(len(cur)):
        if i >= len(prev):
            table[i]["to_prev"] = np.eye(3, 4, dtype=np.float32).reshape(12)
            table[i]["normal_to_prev"] = np.eye(3, dtype=np.float32).reshape(9)
            table[i]["flags"] = MOTION_MOVED | MOTION_DROP
            continue
        a, b = np.ascontiguousarray(prev[i]["transform"], np.float32), np.ascontiguousarray(cur[i]["transform"], np.float32)
        e = np.zeros((), INSTANCE_MOTION)
        st = lib.skh_instance_motion_from_transforms(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p))
        if st != 0:
            raise RuntimeError("skh_instance_motion_from_transforms failed")
        table[i] = e
    return table


RECTIFY_PARAMS = np.dtype([("width", np.uint32), ("height", np.uint32), ("radius", np.uint32), ("k", np.float32), ("albedo_floor", np.float32), ("flags", np.uint32),
                           ("reserved", np.uint32, 8)])  # skh_rectify_params, 56 B
assert RECTIFY_PARAMS.itemsize == 56
RECTIFY_REMODULATE, RECTIFY_SHORTEN = 1, 2
# the defaults of rectify_params (DESIGN.md section 2 "History rectification"; the figures are from the table in docs/LOG.md, "History rectification")
RECTIFY_RADIUS = 1            # 3 x 3.  Error on the changed / unchanged region 8 frames after the step: 0.0203 / 0.0116; radius 2 0.0230 / 0.0118, radius 3 0.0254 / 0.0147, at 2.4 and 4.2 x the time
RECTIFY_K = 2.0               # k 1: 0.0146 / 0.0152, 11.9 % of the unchanged pixels clamped every frame (k 2: 1.5 %); k 3: 0.0248 / 0.0109
RECTIFY_FAST_HISTORY = 4.0    # the fast history's max_history; with 8: 0.0361 / 0.0105 (it still holds the old shadow itself)
RECTIFY_SHORTEN_DEFAULT = True  # without it a clamped pixel keeps alpha 1 / 32: 0.0250 / 0.0108; today's skh_temporal alone: 0.0500 / 0.0111


def rectify_params(width, height, radius=RECTIFY_RADIUS, k=RECTIFY_K, shorten=RECTIFY_SHORTEN_DEFAULT, albedo_floor=DENOISE_ALBEDO_FLOOR, remodulate=True):
    """skh_rectify_params.  The fast history skh_rectify reads is what temporal_params(..., max_history=RECTIFY_FAST_HISTORY) makes skh_temporal write from the
    previous fast history; `remodulate` goes with a temporal call that demodulated."""
    p = np.zeros((), RECTIFY_PARAMS)
    p["width"], p["height"], p["radius"], p["k"], p["albedo_floor"] = width, height, radius, k, albedo_floor
    p["flags"] = (RECTIFY_REMODULATE if remodulate else 0) | (RECTIFY_SHORTEN if shorten else 0)
    return p


VDENOISE_PARAMS = np.dtype([("width", np.uint32), ("height", np.uint32), ("first_level", np.uint32), ("levels", np.uint32), ("sigma_luminance", np.float32),
                            ("sigma_normal", np.float32), ("sigma_plane", np.float32), ("albedo_floor", np.float32), ("epsilon", np.float32),
                            ("min_history", np.float32), ("flags", np.uint32), ("reserved", np.uint32, 5)])  # skh_vdenoise_params, 64 B
assert VDENOISE_PARAMS.itemsize == 64
VDENOISE_ESTIMATE = 4
# the defaults of vdenoise_params (DESIGN.md section 2 "Variance guidance" gives the reasons)
VDENOISE_SIGMA_LUMINANCE = 0.25   # the luminance term is 1 at a quarter of the local per-sample standard deviation: the best on the Cornell orbit (docs/LOG.md); Schied et al. use 4
VDENOISE_MIN_HISTORY = 4.0        # moments younger than this take the spatial estimate
VDENOISE_EPSILON_FRACTION = 1e-2  # epsilon as a fraction of the image's mean demodulated luminance


def luminance(c):
    c = np.asarray(c, np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def vdenoise_epsilon(image, guides=None, albedo_floor=DENOISE_ALBEDO_FLOOR, demodulate=True):
    """the default epsilon for an (h, w, 4) image: VDENOISE_EPSILON_FRACTION x the mean luminance of the filter's first-level input over the pixels it works on
    (denoise_sigma_color's selection of pixels and units)"""
    with np.errstate(invalid="ignore"):
        c = np.asarray(image, np.float64)[..., :3]
    ok = np.isfinite(c).all(axis=-1)
    if guides is not None and guides.get("ids") is not None:
        kind = np.asarray(guides["ids"])[..., 3]
        ok &= (kind == 1) | (kind == 2)
    if demodulate and guides is not None and guides.get("albedo") is not None:
        a = np.asarray(guides["albedo"], np.float64)[..., :3]
        with np.errstate(all="ignore"):
            c = c / np.where(a > albedo_floor, a, albedo_floor)
    level = float(np.abs(luminance(c[ok])).mean()) if ok.any() else 0.0
    return VDENOISE_EPSILON_FRACTION * level if level > 0.0 and np.isfinite(level) else VDENOISE_EPSILON_FRACTION


def vdenoise_params(width, height, levels=5, sigma_luminance=VDENOISE_SIGMA_LUMINANCE, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_plane=None, first_level=0,
                    albedo_floor=DENOISE_ALBEDO_FLOOR, epsilon=None, min_history=VDENOISE_MIN_HISTORY, demodulate=True, remodulate=True, estimate=True, image=None,
                    guides=None, exposure=None, scene=None):
    """skh_vdenoise_params.  sigma_normal, sigma_plane and albedo_floor are denoise_params' (sigma_plane None: DENOISE_PLANE_FRACTION of scene_diagonal(`scene`)).
    epsilon None: vdenoise_epsilon(`image`, `guides`) when the image to be filtered is given, else VDENOISE_EPSILON_FRACTION of 1 / the mean exposure factor, the
    level denoise_params assumes for an image it never sees."""
    p = np.zeros((), VDENOISE_PARAMS)
    p["width"], p["height"], p["first_level"], p["levels"] = width, height, first_level, levels
    if epsilon is None and image is not None:
        epsilon = vdenoise_epsilon(image, guides, albedo_floor, demodulate)
    if epsilon is None:
        e = np.asarray(default_exposure() if exposure is None else exposure, np.float64).reshape(-1)
        epsilon = VDENOISE_EPSILON_FRACTION / float(e.mean())
    if sigma_plane is None:
        if scene is None:
            raise ValueError("sigma_plane is in scene units: give it, or give `scene` to take it as a fraction of the bounding-box diagonal")
        sigma_plane = DENOISE_PLANE_FRACTION * scene_diagonal(scene)
    p["sigma_luminance"], p["sigma_normal"], p["sigma_plane"], p["albedo_floor"] = sigma_luminance, sigma_normal, sigma_plane, albedo_floor
    p["epsilon"], p["min_history"] = epsilon, min_history
    p["flags"] = (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_REMODULATE if remodulate else 0) | (VDENOISE_ESTIMATE if estimate else 0)
    return p


def default_exposure(filmIso=100.0, cm2_factor=1.0, fStop=4.0, shutterSpeed=100.0):
    """exposureValue of OptiXRender::render (OptixRender.cpp:961-987), fp32 arithmetic."""
    f = np.float32
    e = np.array([1.0, 1.0, 1.0], f)
    lum = f(f(e[0] * f(0.299) + e[1] * f(0.587)) + e[2] * f(0.114))
    if filmIso > 0.0:
        e = e * f(f(f(f(cm2_factor) * f(filmIso)) / f(f(f(shutterSpeed) * f(fStop)) * f(fStop))) / f(100.0))
    else:
        e = e * f(cm2_factor)
    inv = f(1.0) / lum
    return (e * inv).astype(f)
