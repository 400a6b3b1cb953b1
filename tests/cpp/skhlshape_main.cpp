// Stand-alone host program over strelka_amd/csrc/skh_lshape.h (no HIP header): the functions k_shade's LSHAPE builds call.
// stdin, one query per line:   s <c> <cos_outer> <cos_inner> <focus>            -> s(c)
//                              k <ux>                                           -> sector, u'
//                              p <ux> <uy> <O xyz> <X xyz> <Y xyz>              -> sector, point xyz, area
// Floats travel as their bit patterns in hex, so that nothing is rounded on the way in or out.
#include <cstdio>
#include <cstring>
#include "skh_lshape.h"

static float f(unsigned u)
{
    float x;
    memcpy(&x, &u, 4);
    return x;
}
static unsigned b(float x)
{
    unsigned u;
    memcpy(&u, &x, 4);
    return u;
}

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1)
    {
        unsigned a[11];
        if (kind == 's')
        {
            if (scanf("%x %x %x %x", a, a + 1, a + 2, a + 3) != 4)
                return 1;
            printf("%08x\n", b(skh::lshape_s(f(a[0]), f(a[1]), f(a[2]), f(a[3]))));
        }
        else if (kind == 'k')
        {
            if (scanf("%x", a) != 1)
                return 1;
            uint32_t k;
            float up;
            skh::lshape_sector(f(a[0]), k, up);
            printf("%u %08x\n", k, b(up));
        }
        else if (kind == 'p')
        {
            for (int i = 0; i < 11; ++i)
                if (scanf("%x", a + i) != 1)
                    return 1;
            const float O[3] = { f(a[2]), f(a[3]), f(a[4]) }, X[3] = { f(a[5]), f(a[6]), f(a[7]) }, Y[3] = { f(a[8]), f(a[9]), f(a[10]) };
            float p[3];
            const uint32_t k = skh::lshape_disc_point(O, X, Y, f(a[0]), f(a[1]), p);
            printf("%u %08x %08x %08x %08x\n", k, b(p[0]), b(p[1]), b(p[2]), b(skh::lshape_disc_area(X, Y)));
        }
        else
            return 2;
    }
    return 0;
}
