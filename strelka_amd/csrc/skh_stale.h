// skh_stale.h -- which derived state of a context each change of an input invalidates: ONE table, and the function that applies a row of it.  No HIP in here
// (tests/cpp/stale_table.cpp prints the table on the host; tests/test_stale_table.py holds it to the matrix).
//
// A setter makes one call -- touched(c, IN_...) in skh_host.h -- where it used to set the flags of everything that depends on what it changed.  Where the flags
// are CLEARED again is not in here: skh_build_accel and the in-place updates, emit_ensure, cut_ensure and lshape_ensure do that, each for what it has just derived.
#pragma once
#include <cstdint>

namespace skh_stale
{
// what a caller can change
enum Input
{
    IN_GEOMETRY = 0,      // skh_set_geometry
    IN_CURVES,            // skh_set_curves
    IN_INSTANCES,         // skh_set_instances
    IN_LIGHTS,            // skh_set_lights
    IN_TEXTURES,          // skh_set_textures
    IN_MATERIALS,         // skh_set_materials
    IN_EMISSION,          // skh_set_emission: a table set, or one removed that existed
    IN_MATERIAL_TEXTURES, // skh_set_material_textures
    IN_MATERIAL_CUTOUTS,  // skh_set_material_cutouts
    IN_MATERIAL_BLEND,    // skh_set_material_blend
    IN_LIGHT_SHAPES,      // skh_set_light_shapes: a table set, or one removed that existed
    IN_REBUILD_OPTION,    // skh_set_option of an option a hierarchy depends on
    IN_UPDATED_INSTANCES, // skh_update_accel given an instance table that it takes in place
    IN_FAILED_UPDATE,     // an in-place update or refit that failed half way: no hierarchy is left behind, the next call builds
    IN_COUNT
};

// what is derived from the inputs, one flag each
enum Derived
{
    D_ACCEL_BUILT = 0,       // the hierarchies are those of the inputs (ensure_ready builds when not)
    D_REFIT_READY,           // the last build left its refit tables behind, and the options are the ones it ran with
    D_UPDATE_READY,          // the last skh_build_accel ran to its end
    D_VERTS_EDITED,          // vertices changed since the last build / refit / update
    D_CURVE_POINTS_EDITED,   // curve control points or radii likewise
    D_EMIT_STALE,            // the emitter table (emit_ensure)
    D_CUT_STALE,             // which cutout and blend entries are in use (cut_ensure)
    D_LSHAPE_STALE,          // which light-shape entries are in use (lshape_ensure)
    D_COUNT
};

// the value a flag takes when its state is invalidated: the "ready" flags fall, the "edited" / "stale" flags rise
constexpr bool kInvalidValue[D_COUNT] = { false, false, false, true, true, true, true, true };

constexpr uint32_t bit(Derived d)
{
    return 1u << d;
}

// the dependency matrix: per input, the derived states it invalidates
constexpr uint32_t kInvalidates[IN_COUNT] = {
    /* IN_GEOMETRY          */ bit(D_ACCEL_BUILT) | bit(D_VERTS_EDITED) | bit(D_EMIT_STALE),
    /* IN_CURVES            */ bit(D_ACCEL_BUILT) | bit(D_CURVE_POINTS_EDITED),
    /* IN_INSTANCES         */ bit(D_ACCEL_BUILT) | bit(D_EMIT_STALE) | bit(D_CUT_STALE),
    /* IN_LIGHTS            */ bit(D_LSHAPE_STALE), // (which shape entries are in use depends on the lights' types and count)
    /* IN_TEXTURES          */ bit(D_CUT_STALE),
    /* IN_MATERIALS         */ bit(D_EMIT_STALE) | bit(D_CUT_STALE),
    /* IN_EMISSION          */ bit(D_EMIT_STALE) | bit(D_CUT_STALE),
    /* IN_MATERIAL_TEXTURES */ 0u,
    /* IN_MATERIAL_CUTOUTS  */ bit(D_CUT_STALE),
    /* IN_MATERIAL_BLEND    */ bit(D_CUT_STALE),
    /* IN_LIGHT_SHAPES      */ bit(D_LSHAPE_STALE),
    /* IN_REBUILD_OPTION    */ bit(D_ACCEL_BUILT) | bit(D_REFIT_READY),
    /* IN_UPDATED_INSTANCES */ bit(D_EMIT_STALE) | bit(D_CUT_STALE), // (the emitter table is in world space: it moves with the instances)
    /* IN_FAILED_UPDATE     */ bit(D_ACCEL_BUILT) | bit(D_REFIT_READY) | bit(D_UPDATE_READY),
};

// applies a row: flag[d] points at the flag of derived state d
inline void apply(Input in, bool* const flag[D_COUNT])
{
    for (int d = 0; d < D_COUNT; ++d)
        if (kInvalidates[in] & (1u << d))
            *flag[d] = kInvalidValue[d];
}
} // namespace skh_stale
