"""A fixed matrix of small renders that reaches every row of the host's kernel dispatch: three scenes (Cornell, a kitchen stand-in with few instances, a hair
stand-in with few strands), each plain and with an environment, emitters, material textures, a cutout, a blend entry and a light shape; one adaptive call, one
skh_render_aovs call and one skh_trace call per mode.  Run once per library under
    rocprofv3 --kernel-trace --stats -- python tools/launch_census.py          (SKH_LIB selects the library; no counters in the same run)
and compare the tables of kernel name x call count: equal tables mean every dispatch row reaches the build it reached before (docs/LOG.md, round 8).
Prints the launch counters of skh_get_stats per case as a cross-check."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from strelka_amd import capi, scene as S, scenes

W = H = 128
SPP, DEPTH = 2, 4


def first_mesh_material(arr):
    inst = arr["instances"]
    mid = int(inst["material_id"][inst["type"] == S.INSTANCE_MESH][0])
    return 0 if mid == 0xFFFFFFFF else mid


def variants(arr):
    n_mat, n_light = len(arr["materials"]), len(arr["lights"])
    m = first_mesh_material(arr)
    rs = np.random.RandomState(5)
    tex = [rs.randint(0, 256, (8, 8, 4)).astype(np.uint8)]
    yield "plain", {}
    yield "environment", {"environment": {"rgb": rs.uniform(0.1, 1.0, (8, 16, 3)).astype(np.float32)}}
    le = np.zeros((n_mat, 3), np.float32)
    le[m] = (2.0, 1.5, 1.0)
    yield "emitters", {"emission": le}
    mt = np.zeros(n_mat, S.MATERIAL_TEXTURES)
    mt["roughness_scale"] = mt["metallic_scale"] = 1.0
    mt["roughness_texture"][m] = len(arr.get("textures") or []) + 1
    yield "material textures", {"textures": list(arr.get("textures") or []) + tex, "material_textures": mt}
    cut = np.zeros(n_mat, S.MATERIAL_CUTOUT)  # (constant opacity 1 against a threshold of 0.5: in use, cuts nothing)
    cut["opacity_channel"], cut["opacity_bias"][m], cut["threshold"][m] = 3, 1.0, 0.5
    yield "cutout", {"material_cutouts": cut}
    bl = np.zeros(n_mat, S.MATERIAL_BLEND)  # (constant opacity 0.5)
    bl["opacity_channel"], bl["opacity_bias"][m], bl["active"][m] = 3, 0.5, 1
    yield "blend", {"material_blend": bl}
    ls = np.zeros(n_light, S.LIGHT_SHAPE)
    ls["flags"], ls["cos_outer"], ls["cos_inner"], ls["axis"] = S.LIGHT_SHAPE_CONE, 0.2, 0.6, (0.0, -1.0, 0.0)
    yield "light shape", {"light_shapes": ls}


def main():
    cases = [("cornell", scenes.cornell_box()), ("kitchen", scenes.kitchen_standin(n_meshes=8, n_instances=24, tri_lo=50, tri_hi=400)),
             ("hair", scenes.hair_standin(n_strands=300))]
    keys = ("launches_trace_closest", "launches_trace_shadow", "launches_shade", "launches_other")
    for name, sc in cases:
        base = sc.arrays()
        cam = sc.getCamera()
        p = S.frame_params(cam, W, H, subframe_index=0, spp_total=SPP, max_depth=DEPTH)
        for what, extra in variants(base):
            arr = dict(base)
            arr.update(extra)
            c = capi.Context(0)
            c.set_scene(arr)
            c.resize(W, H)
            c.reset_stats()
            c.render_subframes(p, SPP)
            st = c.stats()
            print("%-8s %-18s" % (name, what), [st[k] for k in keys], "accumulator sum %.6g" % float(c.read_accum()[..., :3].astype(np.float64).sum()))
            c.close()
    sc = cases[0][1]
    c = capi.Context(0)
    c.set_scene(sc.arrays())
    c.resize(W, H)
    c.set_adaptive(threshold=0.05, min_samples=2, interval=2)
    c.render_subframes(S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=8, max_depth=DEPTH), 8)
    print("adaptive", c.adaptive_info())
    c.set_adaptive(None)
    c.render_aovs(S.aov_params(sc.getCamera(), W, H))
    rays = scenes.random_rays(4096, 1, -0.9, 0.9)
    for mode in (0, 1):
        hits = c.trace(rays, mode)
        print("trace mode %d: %d of %d rays hit" % (mode, int((hits["t"] >= 0).sum()), len(rays)))
    c.close()


if __name__ == "__main__":
    main()
