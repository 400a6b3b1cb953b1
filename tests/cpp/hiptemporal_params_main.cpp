// HipRender's parameter mapping for temporal accumulation (integration/HipRender.h: hipTemporalParams) with the C header and the library alone, no GPU:
//   stdin, one case per line:  normalMin planeTolerance planeFraction maxHistory albedoFloor width height initialLength sceneDiagonal withMatrix
//   stdout, per case:          the 32 words of the skh_temporal_params, hex, and skh_temporal_check's status
// withMatrix 1: prev_world_to_clip is 1, 2, ... 16; 0: no previous frame.  First line: sizeof(skh_temporal_params) sizeof(skh_temporal_info)
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstring>

int main()
{
    printf("%zu %zu\n", sizeof(skh_temporal_params), sizeof(skh_temporal_info));
    char line[512];
    while (fgets(line, sizeof(line), stdin))
    {
        oka::HipTemporal t;
        unsigned w = 0, h = 0, withMatrix = 0;
        float initial = 0.0f, diag = 0.0f;
        if (sscanf(line, "%f %f %f %f %f %u %u %f %f %u", &t.normalMin, &t.planeTolerance, &t.planeFraction, &t.maxHistory, &t.albedoFloor, &w, &h, &initial, &diag, &withMatrix) != 10)
            continue;
        float m[16];
        for (int k = 0; k < 16; ++k)
            m[k] = (float)(k + 1);
        const skh_temporal_params p = oka::hipTemporalParams(t, w, h, withMatrix ? m : nullptr, initial, diag);
        uint32_t words[32];
        memcpy(words, &p, sizeof(words));
        for (uint32_t x : words)
            printf("%08x ", x);
        printf("%d\n", (int)skh_temporal_check(&p));
    }
    return 0;
}
