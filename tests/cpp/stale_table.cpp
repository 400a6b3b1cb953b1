// Prints the dependency table of csrc/skh_stale.h, one row per input: "<input>: <derived>=<0|1> ..." with the value apply() leaves in each flag it touches
// (tests/test_stale_table.py compares the output with the matrix).  Host compiler only: the header has no HIP in it.
#include "skh_stale.h"

#include <cstdio>

using namespace skh_stale;

static const char* input_name(Input in)
{
    switch (in)
    {
    case IN_GEOMETRY: return "set_geometry";
    case IN_CURVES: return "set_curves";
    case IN_INSTANCES: return "set_instances";
    case IN_LIGHTS: return "set_lights";
    case IN_TEXTURES: return "set_textures";
    case IN_MATERIALS: return "set_materials";
    case IN_EMISSION: return "set_emission";
    case IN_MATERIAL_TEXTURES: return "set_material_textures";
    case IN_MATERIAL_CUTOUTS: return "set_material_cutouts";
    case IN_MATERIAL_BLEND: return "set_material_blend";
    case IN_LIGHT_SHAPES: return "set_light_shapes";
    case IN_REBUILD_OPTION: return "rebuild_option";
    case IN_UPDATED_INSTANCES: return "update_accel_instances";
    case IN_FAILED_UPDATE: return "failed_update";
    case IN_COUNT: break;
    }
    return "?";
}

static const char* derived_name(Derived d)
{
    switch (d)
    {
    case D_ACCEL_BUILT: return "accel_built";
    case D_REFIT_READY: return "refit_ready";
    case D_UPDATE_READY: return "update_ready";
    case D_VERTS_EDITED: return "verts_edited";
    case D_CURVE_POINTS_EDITED: return "curve_points_edited";
    case D_EMIT_STALE: return "emit_stale";
    case D_CUT_STALE: return "cut_stale";
    case D_LSHAPE_STALE: return "lshape_stale";
    case D_COUNT: break;
    }
    return "?";
}

int main()
{
    for (int in = 0; in < IN_COUNT; ++in)
    {
        // every flag starts at the value apply() would NOT give it: a flag that differs afterwards was touched, and the row shows what it became
        bool value[D_COUNT];
        bool* flag[D_COUNT];
        for (int d = 0; d < D_COUNT; ++d)
            value[d] = !kInvalidValue[d], flag[d] = &value[d];
        apply((Input)in, flag);
        printf("%s:", input_name((Input)in));
        for (int d = 0; d < D_COUNT; ++d)
            if (value[d] == kInvalidValue[d])
                printf(" %s=%d", derived_name((Derived)d), value[d] ? 1 : 0);
        printf("\n");
    }
    return 0;
}
