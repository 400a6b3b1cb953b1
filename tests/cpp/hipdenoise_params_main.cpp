// HipRender's parameter mapping for the denoiser (integration/HipRender.h: hipDenoiseParams) with the C header and the library alone, no GPU:
//   stdin, one case per line:  levels sigmaColor sigmaNormal sigmaPlane planeFraction albedoFloor width height e0 e1 e2 sceneDiagonal   (floats as %a / decimal)
//   stdout, per case:          the 16 words of the skh_denoise_params, hex, and skh_denoise_check's status
// first line: sizeof(skh_denoise_params) sizeof(skh_denoise_info)
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstring>

int main()
{
    printf("%zu %zu\n", sizeof(skh_denoise_params), sizeof(skh_denoise_info));
    char line[512];
    while (fgets(line, sizeof(line), stdin))
    {
        oka::HipDenoise d;
        unsigned levels = 0, w = 0, h = 0;
        float e[3], diag = 0.0f;
        if (sscanf(line, "%u %f %f %f %f %f %u %u %f %f %f %f", &levels, &d.sigmaColor, &d.sigmaNormal, &d.sigmaPlane, &d.planeFraction, &d.albedoFloor, &w, &h, &e[0], &e[1],
                   &e[2], &diag) != 12)
            continue;
        d.levels = levels;
        const skh_denoise_params p = oka::hipDenoiseParams(d, w, h, e, diag);
        uint32_t words[16];
        memcpy(words, &p, sizeof(words));
        for (uint32_t x : words)
            printf("%08x ", x);
        printf("%d\n", (int)skh_denoise_check(&p));
    }
    return 0;
}
