// HipRender's parameter mapping for history rectification (integration/HipRender.h: HipRectify, hipRectifyParams) with the C header and the library alone, no GPU:
//   stdin, one case per line:  radius k fastHistory shorten width height albedoFloor
//   stdout, per case:          the 14 words of the skh_rectify_params, hex, the fast history's max_history (a float's word, hex), skh_rectify_check's status and
//                              skh_temporal_check's status of a default temporal record with that max_history
// First line: sizeof(skh_rectify_params) sizeof(skh_rectify_info), then the same for a default-constructed HipRectify at 1920 x 1080 with the floor 0.05
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstring>

static void show(const oka::HipRectify& r, unsigned w, unsigned h, float floor)
{
    float fast = 0.0f;
    const skh_rectify_params p = oka::hipRectifyParams(r, w, h, floor, &fast);
    uint32_t words[14], fw;
    memcpy(words, &p, sizeof(words));
    memcpy(&fw, &fast, 4);
    for (uint32_t x : words)
        printf("%08x ", x);
    skh_temporal_params t = oka::hipTemporalParams(oka::HipTemporal(), w ? w : 1u, h ? h : 1u, nullptr, 1.0f, 1.0f);
    t.max_history = fast;
    printf("%08x %d %d\n", fw, (int)skh_rectify_check(&p), (int)skh_temporal_check(&t));
}

int main()
{
    static_assert(sizeof(skh_rectify_params) == 56, "ABI layout");
    printf("%zu %zu\n", sizeof(skh_rectify_params), sizeof(skh_rectify_info));
    show(oka::HipRectify(), 1920, 1080, 0.05f);
    char line[512];
    while (fgets(line, sizeof(line), stdin))
    {
        oka::HipRectify r;
        unsigned w = 0, h = 0, shorten = 0;
        float floor = 0.0f;
        if (sscanf(line, "%u %f %f %u %u %u %f", &r.radius, &r.k, &r.fastHistory, &shorten, &w, &h, &floor) != 7)
            continue;
        r.shorten = shorten != 0;
        show(r, w, h, floor);
    }
    return 0;
}
