// skh_aov_check through the C header and the library alone (no Python binding, no GPU):
//   skhaov < lines
// every line: image_w image_h, then the 60 words of an skh_aov_params record in hex (or the word NULL for a null pointer); prints one status per line.
// The first line printed is sizeof(skh_aov_params), sizeof(skh_aov_info), SKH_AOV_COUNT and SKH_AOV_PIXEL_CENTRE, as the header gives them.
#include "strelka_hip.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    static_assert(sizeof(skh_aov_params) == 60 * sizeof(uint32_t), "60 words");
    printf("%zu %zu %u %x\n", sizeof(skh_aov_params), sizeof(skh_aov_info), SKH_AOV_COUNT, SKH_AOV_PIXEL_CENTRE);
    std::string line;
    while (std::getline(std::cin, line))
    {
        if (line.empty())
            continue;
        std::istringstream in(line);
        uint32_t w = 0, h = 0;
        in >> std::dec >> w >> h;
        std::string first;
        in >> first;
        if (first == "NULL")
        {
            printf("%d\n", (int)skh_aov_check(nullptr, w, h));
            continue;
        }
        uint32_t words[60];
        words[0] = (uint32_t)std::stoul(first, nullptr, 16);
        bool ok = true;
        for (int k = 1; k < 60; ++k)
        {
            std::string t;
            if (!(in >> t))
            {
                ok = false;
                break;
            }
            words[k] = (uint32_t)std::stoul(t, nullptr, 16);
        }
        if (!ok)
        {
            fprintf(stderr, "a short line\n");
            return 2;
        }
        skh_aov_params p;
        memcpy(&p, words, sizeof(p));
        printf("%d\n", (int)skh_aov_check(&p, w, h));
    }
    return 0;
}
