// HipRender's parameter mapping for variance guidance (integration/HipRender.h: hipVarianceParams) with the C header and the library alone, no GPU:
//   stdin, one case per line:  sigmaLuminance epsilon minHistory levels sigmaNormal sigmaPlane albedoFloor width height ex0 ex1 ex2 sceneDiagonal
//   stdout, per case:          the 16 words of the skh_vdenoise_params, hex, and skh_vdenoise_check's status
// First line: sizeof(skh_vdenoise_params) sizeof(skh_vdenoise_info) sizeof(skh_moments_info)
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstring>

int main()
{
    printf("%zu %zu %zu\n", sizeof(skh_vdenoise_params), sizeof(skh_vdenoise_info), sizeof(skh_moments_info));
    char line[512];
    while (fgets(line, sizeof(line), stdin))
    {
        oka::HipVariance v;
        oka::HipDenoise d;
        unsigned w = 0, h = 0;
        float ex[3], diag = 0.0f;
        if (sscanf(line, "%f %f %f %u %f %f %f %u %u %f %f %f %f", &v.sigmaLuminance, &v.epsilon, &v.minHistory, &d.levels, &d.sigmaNormal, &d.sigmaPlane, &d.albedoFloor, &w, &h,
                   &ex[0], &ex[1], &ex[2], &diag) != 13)
            continue;
        const skh_vdenoise_params p = oka::hipVarianceParams(v, d, w, h, ex, diag);
        uint32_t words[16];
        memcpy(words, &p, sizeof(words));
        for (uint32_t x : words)
            printf("%08x ", x);
        printf("%d\n", (int)skh_vdenoise_check(&p));
    }
    return 0;
}
