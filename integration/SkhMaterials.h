// MaterialDescription -> skh_material, for builds against the REAL Strelka headers (-DSKH_WITH_STRELKA_HEADERS).
//
// The reference compiles every oka::Scene::MaterialDescription {file, name, params[{type, name, value bytes}]} to MDL PTX plus an
// argument block (src/render/optix/OptixRender.cpp:1270-1433, materialmanager.cpp:524-609).  Here the block is the fixed 64-byte
// skh_material (include/strelka_hip.h) and this header is the translation -- the C++ statement of
// strelka_amd/scene_io.py::material_from_description, which the tests pin (tests/test_scene_io.py, tests/test_gltf.py):
//   default.mdl::default_material.diffuse_color          (OptixRender.cpp:1090-1097, HdStrelka/RenderPass.cpp:222-245)  -> SKH_MAT_DIFFUSE
//   OmniPBR.{diffuse_color_constant, reflection_roughness_constant, metallic_constant, diffuse_texture, normalmap_texture}
//                                                         (sceneloader/gltfloader.cpp:304-352)                            -> SKH_MAT_PBR
//           its roughness / metallic / ORM / emissive maps                                                               -> skh_material_textures (materialTextures below)
//           enable_opacity + opacity_threshold [opacity_texture]; UsdPreviewSurface opacityThreshold                       -> skh_material_cutout (materialCutout below)
//           enable_opacity without a threshold; UsdPreviewSurface opacity < 1 without one (behind HipRender::setAlphaBlend)   -> skh_material_blend (materialBlend below)
//   OmniGlass.{glass_color, glass_ior, frosting_roughness} (gltfloader.cpp:354-406)                                      -> SKH_MAT_GLASS
//   UsdPreviewSurface parameter sets (HdStrelka's eMaterialX descriptions, HdStrelka/Material.cpp:52-150)                -> PBR | GLASS
//   names containing "hair" (the `hair` sub-expression, materialmanager/mdlPtxCodeGen.cpp:143-155)                       -> SKH_MAT_HAIR
// The functions are templates over the description type -- anything with {file, name, params[{type, name, value}]} and the reference's
// Param::Type numbering (eFloat 0, eInt 1, eBool 2, eFloat2 3, eFloat3 4, eFloat4 5, eTexture 6: materialmanager.h:35-44) -- so that
// tests/test_integration_files.py can run them on a local look-alike of the reference's two structs and compare every case with the
// Python statement; inside the Strelka tree they are instantiated with oka::Scene::MaterialDescription itself (HipRender.cpp).
#pragma once
#ifdef SKH_WITH_STRELKA_HEADERS
#    include <strelka_hip.h>
#else
#    include "../include/strelka_hip.h"
#endif

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <string>

namespace oka
{
namespace skhmat
{
enum : uint32_t
{
    kFloat = 0,
    kInt = 1,
    kBool = 2,
    kFloat2 = 3,
    kFloat3 = 4,
    kFloat4 = 5,
    kTexture = 6
};

template <class Desc>
inline auto find(const Desc& d, const char* name) -> decltype(&d.params[0])
{
    for (const auto& p : d.params)
        if (p.name == name)
            return &p;
    return nullptr;
}
template <class Desc>
inline float scalar(const Desc& d, const char* name, float def)
{
    const auto* p = find(d, name);
    if (!p)
        return def;
    if ((uint32_t)p->type == kBool)
        return (!p->value.empty() && p->value[0]) ? 1.0f : 0.0f;
    if (p->value.size() < sizeof(float))
        return def;
    if ((uint32_t)p->type == kInt)
    {
        int v;
        memcpy(&v, p->value.data(), sizeof(v));
        return (float)v;
    }
    float v;
    memcpy(&v, p->value.data(), sizeof(v));
    return v;
}
template <class Desc>
inline void color(const Desc& d, const char* name, float out[3], float r, float g, float b)
{
    out[0] = r, out[1] = g, out[2] = b;
    const auto* p = find(d, name);
    if (p && p->value.size() >= 3 * sizeof(float))
        memcpy(out, p->value.data(), 3 * sizeof(float));
}
// the path of an eTexture parameter ("" if the material has none); the caller loads it (stbi_load(..., STBI_rgb_alpha), resolved
// against `resource/searchPath` as OptixRender.cpp:1346-1362 does) and passes the 1-based texture id back in
template <class Desc>
inline std::string texturePath(const Desc& d, const char* name)
{
    const auto* p = find(d, name);
    if (!p || (uint32_t)p->type != kTexture)
        return std::string();
    return std::string(reinterpret_cast<const char*>(p->value.data()), p->value.size());
}

template <class Desc>
// `alphaBlend` (HipRender::setAlphaBlend, off by default): a UsdPreviewSurface whose opacity is a blend entry's (materialBlend below) is PBR, not glass.
inline skh_material translate(const Desc& d, uint32_t diffuseTextureId = 0, uint32_t normalTextureId = 0, bool alphaBlend = false)
{
    skh_material m;
    memset(&m, 0, sizeof(m));
    m.base_color[0] = m.base_color[1] = m.base_color[2] = 0.8f;
    m.roughness = 0.5f, m.specular = 0.5f, m.ior = 1.5f;
    std::string low = d.name + " " + d.file;
    std::transform(low.begin(), low.end(), low.begin(), [](unsigned char c) { return (char)tolower(c); });
    const bool preview = find(d, "diffuseColor") || find(d, "useSpecularWorkflow") || find(d, "specularColor") || find(d, "clearcoat") ||
                         find(d, "emissiveColor");
    if (preview)
    {
        // UsdPreviewSurface spec defaults: diffuseColor 0.18, roughness 0.5, metallic 0, ior 1.5, opacity 1 (< 0.5 is treated as glass -- unless an
        // opacityThreshold > 0 makes the opacity a cutout's: materialCutout)
        m.type = (scalar(d, "opacity", 1.0f) < 0.5f && !(scalar(d, "opacityThreshold", 0.0f) > 0.0f) && !alphaBlend) ? SKH_MAT_GLASS : SKH_MAT_PBR;
        color(d, "diffuseColor", m.base_color, 0.18f, 0.18f, 0.18f);
        m.roughness = scalar(d, "roughness", 0.5f);
        m.metallic = scalar(d, "metallic", 0.0f);
        m.ior = scalar(d, "ior", 1.5f);
    }
    else if (low.find("glass") != std::string::npos)
    {
        m.type = SKH_MAT_GLASS;
        color(d, "glass_color", m.base_color, 1.0f, 1.0f, 1.0f);
        m.roughness = scalar(d, "frosting_roughness", 0.0f);
        m.ior = scalar(d, "glass_ior", 1.491f); // OmniGlass.mdl default
    }
    else if (low.find("pbr") != std::string::npos)
    {
        m.type = SKH_MAT_PBR;
        color(d, "diffuse_color_constant", m.base_color, 0.2f, 0.2f, 0.2f); // OmniPBR.mdl default
        m.roughness = scalar(d, "reflection_roughness_constant", 0.5f);
        m.metallic = scalar(d, "metallic_constant", 0.0f);
        m.base_color_texture = diffuseTextureId;
        m.normal_texture = normalTextureId;
    }
    else if (low.find("hair") != std::string::npos)
    {
        // df::chiang_hair_bsdf: colour -> absorption by Chiang et al. 2016 eq. 9 when no absorption_coefficient is given
        m.type = SKH_MAT_HAIR;
        const float rn = scalar(d, "roughness_azimuthal", scalar(d, "roughness", 0.3f));
        float sig[3];
        if (find(d, "absorption_coefficient"))
            color(d, "absorption_coefficient", sig, 0.0f, 0.0f, 0.0f);
        else
        {
            float c[3];
            color(d, find(d, "diffuse_color") ? "diffuse_color" : "color", c, 0.35f, 0.2f, 0.1f);
            const double b = rn, dn = 5.969 - 0.215 * b + 2.532 * b * b - 10.73 * b * b * b + 5.574 * b * b * b * b + 0.245 * b * b * b * b * b;
            for (int k = 0; k < 3; ++k)
            {
                const double l = std::log(std::min(1.0, std::max(1e-4, (double)c[k]))) / dn;
                sig[k] = (float)(l * l);
            }
        }
        color(d, "diffuse_reflection_tint", m.base_color, 1.0f, 1.0f, 1.0f);
        m.roughness = scalar(d, "roughness_R", scalar(d, "roughness", 0.3f));
        m.metallic = scalar(d, "roughness_TT", 0.0f);
        m.specular = scalar(d, "roughness_TRT", 0.0f);
        m.ior = scalar(d, "ior", 1.55f);
        m.reserved[0] = sig[0], m.reserved[1] = sig[1], m.reserved[2] = sig[2], m.reserved[3] = rn;
        m.reserved[4] = scalar(d, "cuticle_angle", 0.035f);
        m.reserved[5] = scalar(d, "diffuse_reflection_weight", 0.0f);
    }
    else
    {
        m.type = SKH_MAT_DIFFUSE;
        color(d, "diffuse_color", m.base_color, 0.8f, 0.8f, 0.8f);
    }
    return m;
}

// The radiance Le the description's surfaces emit (skh_set_emission's entry for the material; 0 0 0 = none) -- the C++ statement of
// strelka_amd/scene_io.py::emission_from_description: UsdPreviewSurface emissiveColor; OmniPBR enable_emission ? emissive_color * emissive_intensity : 0.
template <class Desc>
inline void emission(const Desc& d, float out[3])
{
    out[0] = out[1] = out[2] = 0.0f;
    std::string low = d.name + " " + d.file;
    std::transform(low.begin(), low.end(), low.begin(), [](unsigned char c) { return (char)tolower(c); });
    const bool preview = find(d, "diffuseColor") || find(d, "useSpecularWorkflow") || find(d, "specularColor") || find(d, "clearcoat") ||
                         find(d, "emissiveColor");
    if (preview)
        color(d, "emissiveColor", out, 0.0f, 0.0f, 0.0f);
    else if (low.find("glass") == std::string::npos && low.find("pbr") != std::string::npos && scalar(d, "enable_emission", 0.0f) != 0.0f)
    {
        color(d, "emissive_color", out, 1.0f, 1.0f, 1.0f);
        const float k = scalar(d, "emissive_intensity", 1.0f);
        for (int c = 0; c < 3; ++c)
            out[c] *= k;
    }
    for (int c = 0; c < 3; ++c)
        out[c] = out[c] > 0.0f ? out[c] : 0.0f; // (a negative value, or a NaN, does not emit)
}

// The description's roughness / metallic / emission maps (skh_set_material_textures' entry for the material) -- the C++ statement of
// strelka_amd/scene_io.py::material_textures_from_description, OmniPBR only:
//   reflectionroughness_texture + reflection_roughness_texture_influence (default 0)  -> roughness, channel r, scale = influence,
//                                                                                         bias = reflection_roughness_constant * (1 - influence)
//   metallic_texture + metallic_texture_influence                                      -> metallic, likewise
//   enable_ORM_texture + ORM_texture [ORM_roughness_scale, ORM_metallic_scale]         -> roughness = g, metallic = b of one texture (r, occlusion, is ignored)
//   enable_emission + emissive_color_texture | emissive_mask_texture                   -> emission, rgb | channel r (the mask only without a colour texture)
// `textureId(path)` loads the named texture the way the caller loads diffuse_texture and returns its 1-based id (0: not available -> the slot binds nothing).
template <class Desc, class TextureId>
inline skh_material_textures materialTextures(const Desc& d, TextureId&& textureId)
{
    skh_material_textures e;
    memset(&e, 0, sizeof(e));
    e.emission_channel = 4u;
    e.roughness_scale = e.metallic_scale = 1.0f;
    std::string low = d.name + " " + d.file;
    std::transform(low.begin(), low.end(), low.begin(), [](unsigned char c) { return (char)tolower(c); });
    const bool preview = find(d, "diffuseColor") || find(d, "useSpecularWorkflow") || find(d, "specularColor") || find(d, "clearcoat") ||
                         find(d, "emissiveColor");
    if (preview || low.find("glass") != std::string::npos || low.find("pbr") == std::string::npos)
        return e;
    auto id = [&](const char* name) -> uint32_t {
        const std::string path = texturePath(d, name);
        return path.empty() ? 0u : (uint32_t)textureId(path);
    };
    const uint32_t orm = scalar(d, "enable_ORM_texture", 0.0f) != 0.0f ? id("ORM_texture") : 0u;
    if (orm)
    {
        e.roughness_texture = e.metallic_texture = orm;
        e.roughness_channel = 1u, e.metallic_channel = 2u;
        e.roughness_scale = scalar(d, "ORM_roughness_scale", 1.0f);
        e.metallic_scale = scalar(d, "ORM_metallic_scale", 1.0f);
    }
    else
    {
        const float wr = scalar(d, "reflection_roughness_texture_influence", 0.0f), wm = scalar(d, "metallic_texture_influence", 0.0f);
        const uint32_t tr = wr != 0.0f ? id("reflectionroughness_texture") : 0u, tm = wm != 0.0f ? id("metallic_texture") : 0u;
        if (tr)
        {
            const float rest = 1.0f - wr;
            e.roughness_texture = tr, e.roughness_scale = wr, e.roughness_bias = scalar(d, "reflection_roughness_constant", 0.5f) * rest;
        }
        if (tm)
        {
            const float rest = 1.0f - wm;
            e.metallic_texture = tm, e.metallic_scale = wm, e.metallic_bias = scalar(d, "metallic_constant", 0.0f) * rest;
        }
    }
    if (scalar(d, "enable_emission", 0.0f) != 0.0f)
    {
        const uint32_t col = id("emissive_color_texture"), mask = col ? 0u : id("emissive_mask_texture");
        if (col)
            e.emission_texture = col, e.emission_channel = 4u;
        else if (mask)
            e.emission_texture = mask, e.emission_channel = 0u;
    }
    return e;
}

// The description's cutout (skh_set_material_cutouts' entry for the material; threshold 0 = none) -- the C++ statement of
// strelka_amd/scene_io.py::material_cutout_from_description:
//   OmniPBR, enable_opacity and opacity_threshold > 0   -> threshold = opacity_threshold; with enable_opacity_texture and an opacity_texture that loads: that texture,
//                                                          channel a for opacity_mode 0, else r (a simplification: the other mono modes agree on grey maps only),
//                                                          scale = opacity_scale (default 1), bias 0; without one: no look-up, scale 0, bias = opacity_constant (default 1)
//   UsdPreviewSurface, opacityThreshold > 0             -> no texture, scale 0, bias = opacity (default 1), threshold = opacityThreshold
// Thresholds above 1 are clamped to 1.  `textureId(path)` as for materialTextures.
template <class Desc, class TextureId>
inline skh_material_cutout materialCutout(const Desc& d, TextureId&& textureId)
{
    skh_material_cutout e;
    memset(&e, 0, sizeof(e));
    e.opacity_channel = 3u;
    e.opacity_scale = 1.0f;
    std::string low = d.name + " " + d.file;
    std::transform(low.begin(), low.end(), low.begin(), [](unsigned char c) { return (char)tolower(c); });
    const bool preview = find(d, "diffuseColor") || find(d, "useSpecularWorkflow") || find(d, "specularColor") || find(d, "clearcoat") ||
                         find(d, "emissiveColor");
    if (preview)
    {
        const float th = scalar(d, "opacityThreshold", 0.0f);
        if (th > 0.0f)
            e.opacity_scale = 0.0f, e.opacity_bias = scalar(d, "opacity", 1.0f), e.threshold = std::min(th, 1.0f);
        return e;
    }
    if (low.find("glass") != std::string::npos || low.find("pbr") == std::string::npos || scalar(d, "enable_opacity", 0.0f) == 0.0f)
        return e;
    const float th = scalar(d, "opacity_threshold", 0.0f);
    if (!(th > 0.0f))
        return e;
    e.threshold = std::min(th, 1.0f);
    uint32_t t = 0u;
    if (scalar(d, "enable_opacity_texture", 0.0f) != 0.0f)
    {
        const std::string path = texturePath(d, "opacity_texture");
        t = path.empty() ? 0u : (uint32_t)textureId(path);
    }
    if (t)
    {
        e.opacity_texture = t, e.opacity_channel = scalar(d, "opacity_mode", 0.0f) == 0.0f ? 3u : 0u;
        e.opacity_scale = scalar(d, "opacity_scale", 1.0f);
    }
    else
        e.opacity_scale = 0.0f, e.opacity_bias = scalar(d, "opacity_constant", 1.0f);
    return e;
}

// The description's blend entry (skh_set_material_blend's entry for the material; active 0 = none) -- the C++ statement of
// strelka_amd/scene_io.py::material_blend_from_description: the cases materialCutout leaves, an opacity WITHOUT a threshold.
//   OmniPBR, enable_opacity and no opacity_threshold > 0   -> with enable_opacity_texture and an opacity_texture that loads: that texture, channel a for opacity_mode 0,
//                                                             else r, scale = opacity_scale (default 1), bias 0; without one: scale 0, bias = opacity_constant
//                                                             (default 1) -- inactive when that constant is 1 or more
//   UsdPreviewSurface, opacity < 1, no opacityThreshold > 0 -> no texture, scale 0, bias = opacity
template <class Desc, class TextureId>
inline skh_material_blend materialBlend(const Desc& d, TextureId&& textureId)
{
    skh_material_blend e;
    memset(&e, 0, sizeof(e));
    e.opacity_channel = 3u;
    e.opacity_scale = 1.0f;
    std::string low = d.name + " " + d.file;
    std::transform(low.begin(), low.end(), low.begin(), [](unsigned char c) { return (char)tolower(c); });
    const bool preview = find(d, "diffuseColor") || find(d, "useSpecularWorkflow") || find(d, "specularColor") || find(d, "clearcoat") ||
                         find(d, "emissiveColor");
    if (preview)
    {
        const float opacity = scalar(d, "opacity", 1.0f);
        if (opacity < 1.0f && !(scalar(d, "opacityThreshold", 0.0f) > 0.0f))
            e.opacity_scale = 0.0f, e.opacity_bias = opacity, e.active = 1u;
        return e;
    }
    if (low.find("glass") != std::string::npos || low.find("pbr") == std::string::npos || scalar(d, "enable_opacity", 0.0f) == 0.0f ||
        scalar(d, "opacity_threshold", 0.0f) > 0.0f)
        return e;
    uint32_t t = 0u;
    if (scalar(d, "enable_opacity_texture", 0.0f) != 0.0f)
    {
        const std::string path = texturePath(d, "opacity_texture");
        t = path.empty() ? 0u : (uint32_t)textureId(path);
    }
    if (t)
    {
        e.opacity_texture = t, e.opacity_channel = scalar(d, "opacity_mode", 0.0f) == 0.0f ? 3u : 0u;
        e.opacity_scale = scalar(d, "opacity_scale", 1.0f);
        e.active = 1u;
    }
    else
    {
        const float c = scalar(d, "opacity_constant", 1.0f);
        if (c < 1.0f)
            e.opacity_scale = 0.0f, e.opacity_bias = c, e.active = 1u;
    }
    return e;
}
} // namespace skhmat
} // namespace oka
