// Holds csrc/skh_order.h to its properties on the host (tests/test_queue_order_cpu.py runs it per case; it includes nothing of the library but that header, and may
// be built with -fsanitize=address,undefined and run directly).
//
//   queue_order_main W H T batch cell tiles frozen
//     W H T    image size, tile size (a power of two >= 8)
//     batch    sub-frames of the pass
//     cell     cell size: n >= 1 raygen blocks of 512 slots, or -1 = one 64-slot chunk
//     tiles    "all" (row-major over the image, as alloc_frame lists them), or "x,y;x,y;..." (a custom list)
//     frozen   k: every k-th tile (k - 1, 2k - 1, ...) is frozen; 0: none
//
// The per-chunk valid counts and the units' first pixels are derived here the way the library derives them (Morton order inside a tile).  Prints one line
// "OK total=... per=... region=... cells=... runs=a,b,..." or the first property that does not hold, and exits 1.
#include "skh_order.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace skh_order;

static const uint32_t SHARDS = 8;

#define REQUIRE(cond, ...)                                                                                                                                             \
    do                                                                                                                                                                 \
    {                                                                                                                                                                  \
        if (!(cond))                                                                                                                                                   \
        {                                                                                                                                                              \
            printf("FAILED %s: ", #cond);                                                                                                                              \
            printf(__VA_ARGS__);                                                                                                                                       \
            printf("\n");                                                                                                                                              \
            return 1;                                                                                                                                                  \
        }                                                                                                                                                              \
    } while (0)

int main(int argc, char** argv)
{
    if (argc != 8)
    {
        fprintf(stderr, "usage: queue_order_main W H T batch cell tiles frozen\n");
        return 2;
    }
    const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]), T = (uint32_t)atoi(argv[3]), batch = (uint32_t)atoi(argv[4]);
    const int cell = atoi(argv[5]);
    const uint32_t freezeEvery = (uint32_t)atoi(argv[7]);
    uint32_t shift = 0;
    while ((1u << shift) < T)
        ++shift;
    REQUIRE(T >= 8 && (1u << shift) == T && batch >= 1 && (cell == -1 || cell >= 1), "arguments");
    std::vector<uint32_t> tileXY;
    if (strcmp(argv[6], "all") == 0)
    {
        for (uint32_t y = 0; y < H; y += T)
            for (uint32_t x = 0; x < W; x += T)
                tileXY.push_back(x), tileXY.push_back(y);
    }
    else
    {
        for (const char* p = argv[6]; *p;)
        {
            char* end;
            tileXY.push_back((uint32_t)strtoul(p, &end, 10));
            p = (*end == ',' || *end == ';') ? end + 1 : end;
        }
        REQUIRE(tileXY.size() % 2 == 0, "tile list");
    }
    const uint32_t numTiles = (uint32_t)(tileXY.size() / 2), numSlots = numTiles * T * T, shift2 = 2 * shift, mask = (1u << shift2) - 1u;
    std::vector<uint32_t> frozen(numTiles, 0u);
    for (uint32_t t = 0; freezeEvery && t < numTiles; ++t)
        frozen[t] = (t % freezeEvery == freezeEvery - 1u) ? 1u : 0u;

    // valid slots per 64-slot chunk, frozen tiles left out
    const uint32_t chunks = numSlots / 64u, blocks = (numSlots + 511u) / 512u;
    std::vector<uint32_t> chunkValid(chunks, 0u), chunkXY(2 * (size_t)chunks, 0u);
    for (uint32_t j = 0; j < chunks; ++j)
    {
        const uint32_t tile = (j * 64u) >> shift2, m = (j * 64u) & mask;
        const uint32_t x0 = tileXY[2 * tile] + even_bits(m), y0 = tileXY[2 * tile + 1] + even_bits(m >> 1);
        chunkXY[2 * (size_t)j] = x0, chunkXY[2 * (size_t)j + 1] = y0;
        for (uint32_t k = 0; k < 64u && !frozen[tile]; ++k)
            chunkValid[j] += (x0 + even_bits(k) < W && y0 + even_bits(k >> 1) < H) ? 1u : 0u;
    }
    // the slot order's tables as the library has always summed them: per 512-slot block
    std::vector<uint32_t> blockValid(blocks, 0u), blockBase(blocks, 0u);
    uint32_t validPerSub = 0;
    for (uint32_t b = 0; b < blocks; ++b)
    {
        blockBase[b] = validPerSub;
        for (uint32_t j = b * 8u; j < std::min(chunks, (b + 1u) * 8u); ++j)
            blockValid[b] += chunkValid[j];
        validPerSub += blockValid[b];
    }
    uint32_t partial = 0, empty = 0;
    for (uint32_t b = 0; b < blocks; ++b)
        partial += (blockValid[b] > 0u && blockValid[b] < 512u) ? 1u : 0u, empty += blockValid[b] == 0u ? 1u : 0u;

    // ---- queue_order 0: blockBase / validPerSub exactly ----
    {
        Tables t;
        slot_order(blockValid.data(), blocks, t);
        REQUIRE(t.validPerSub == validPerSub, "slot order: %u valid slots per sub-frame, %u expected", t.validPerSub, validPerSub);
        REQUIRE(t.qBase.size() == std::max(1u, blocks) && t.subStride.size() == t.qBase.size(), "slot order: table sizes");
        for (uint32_t b = 0; b < blocks; ++b)
            REQUIRE(t.qBase[b] == blockBase[b] && t.subStride[b] == validPerSub, "slot order: block %u has base %u stride %u, expected %u %u", b, t.qBase[b], t.subStride[b], blockBase[b], validPerSub);
    }

    // ---- queue_order 1 ----
    // the units: blocks, or chunks padded to whole blocks (what k_raygen's waves index)
    const uint32_t nUnits = cell < 0 ? blocks * 8u : blocks, cellUnits = cell < 0 ? 1u : (uint32_t)cell;
    std::vector<uint32_t> valid(nUnits, 0u), origin(2 * (size_t)nUnits, 0u);
    for (uint32_t u = 0; u < nUnits; ++u)
    {
        const uint32_t j0 = cell < 0 ? u : u * 8u;
        if (j0 >= chunks)
            continue;
        valid[u] = cell < 0 ? chunkValid[j0] : blockValid[u];
        origin[2 * (size_t)u] = chunkXY[2 * (size_t)j0], origin[2 * (size_t)u + 1] = chunkXY[2 * (size_t)j0 + 1];
    }
    Tables t;
    cell_order(valid.data(), origin.data(), nUnits, batch, cellUnits, SHARDS, t);
    const uint32_t total = validPerSub * batch;
    REQUIRE(t.validPerSub == validPerSub, "cell order: %u valid slots per sub-frame, %u expected", t.validPerSub, validPerSub);
    REQUIRE(t.qBase.size() == std::max(1u, nUnits) && t.subStride.size() == t.qBase.size(), "cell order: table sizes");
    const uint32_t nCells = (nUnits + cellUnits - 1u) / cellUnits;
    REQUIRE(t.curvePos.size() == nCells && t.runStart.size() == SHARDS + 1u, "cell order: curve / run sizes");

    // (unit, sub, rank) -> position is a bijection onto [0, total)
    std::vector<uint8_t> hit(total, 0u);
    for (uint32_t u = 0; u < nUnits; ++u)
        for (uint32_t s = 0; s < batch; ++s)
            for (uint32_t r = 0; r < valid[u]; ++r)
            {
                const uint64_t pos = (uint64_t)t.qBase[u] + (uint64_t)s * t.subStride[u] + r;
                REQUIRE(pos < total, "unit %u sub %u rank %u goes to %llu of %u", u, s, r, (unsigned long long)pos, total);
                REQUIRE(!hit[pos], "position %llu is taken twice (unit %u sub %u rank %u)", (unsigned long long)pos, u, s, r);
                hit[pos] = 1;
            }
    // (every position is taken: total of them were marked, none twice)

    // every (cell, sub) run is contiguous, in unit order, and the sub-frames of a cell are adjacent
    std::vector<uint32_t> cellValid(nCells, 0u), cellBase(nCells, 0u);
    uint32_t nonEmpty = 0, cellMax = 0;
    for (uint32_t k = 0; k < nCells; ++k)
    {
        uint32_t inCell = 0;
        const uint32_t u0 = k * cellUnits;
        for (uint32_t u = u0; u < std::min(nUnits, u0 + cellUnits); ++u)
        {
            if (valid[u])
                REQUIRE(t.qBase[u] == t.qBase[u0] + inCell, "cell %u: unit %u starts at %u, %u slots behind the cell's start %u expected", k, u, t.qBase[u], inCell, t.qBase[u0]);
            inCell += valid[u];
        }
        cellValid[k] = inCell, cellBase[k] = t.qBase[u0];
        for (uint32_t u = u0; u < std::min(nUnits, u0 + cellUnits); ++u)
            if (valid[u])
                REQUIRE(t.subStride[u] == inCell, "cell %u: unit %u has stride %u, the cell holds %u", k, u, t.subStride[u], inCell);
        REQUIRE((t.curvePos[k] == kNoCell) == (inCell == 0u), "cell %u: %u valid slots, curve position %u", k, inCell, t.curvePos[k]);
        nonEmpty += inCell ? 1u : 0u, cellMax = std::max(cellMax, inCell);
    }

    // the curve: a numbering 0 .. nonEmpty - 1 of the cells with a valid slot along which the Morton key of the first pixel never falls
    std::vector<uint32_t> byPos(nonEmpty, kNoCell);
    for (uint32_t k = 0; k < nCells; ++k)
        if (t.curvePos[k] != kNoCell)
        {
            REQUIRE(t.curvePos[k] < nonEmpty && byPos[t.curvePos[k]] == kNoCell, "cell %u: curve position %u of %u is out of range or taken", k, t.curvePos[k], nonEmpty);
            byPos[t.curvePos[k]] = k;
        }
    for (uint32_t i = 1; i < nonEmpty; ++i)
    {
        const uint32_t a = byPos[i - 1] * cellUnits, b = byPos[i] * cellUnits;
        REQUIRE(morton_key(origin[2 * (size_t)a], origin[2 * (size_t)a + 1]) <= morton_key(origin[2 * (size_t)b], origin[2 * (size_t)b + 1]), "curve positions %u, %u: the Morton key falls", i - 1, i);
    }
    // run g = [runStart[g], runStart[g + 1]) holds exactly the cells at curve positions g, g + 8, ..., in that order, back to back
    REQUIRE(t.runStart[0] == 0u && t.runStart[SHARDS] == total, "runs cover [%u, %u), the queue is [0, %u)", t.runStart[0], t.runStart[SHARDS], total);
    std::string runs;
    for (uint32_t g = 0; g < SHARDS; ++g)
    {
        uint32_t pos = t.runStart[g];
        for (uint32_t i = g; i < nonEmpty; i += SHARDS)
        {
            REQUIRE(cellBase[byPos[i]] == pos, "run %u: the cell at curve position %u starts at %u, %u expected", g, i, cellBase[byPos[i]], pos);
            pos += cellValid[byPos[i]] * batch;
        }
        REQUIRE(pos == t.runStart[g + 1], "run %u ends at %u, the next one starts at %u", g, pos, t.runStart[g + 1]);
        runs += (g ? "," : "") + std::to_string(t.runStart[g + 1] - t.runStart[g]);
    }
    // What a queue region holds is a SHARD: positions [g * per, (g + 1) * per), the cut k_raygen makes whatever the order.  It never outgrows the region of a frame
    // whose pass capacity is `batch` (the smallest capacity this pass fits).  The order's own runs are the shards up to the difference between cells: with C cells
    // of at most cellMax slots a run holds floor or ceil of C / 8 of them, so it is at most ceil(C / 8) * cellMax * batch long.
    const uint32_t per = per_shard(total, SHARDS);
    const uint32_t region = (uint32_t)(((((uint64_t)std::max(1u, numSlots) * batch + SHARDS - 1u) / SHARDS) + 63u) & ~(uint64_t)63u);
    REQUIRE(per <= region, "a shard of %u positions, a region of %u", per, region);
    REQUIRE((uint64_t)per * SHARDS >= total, "%u shards of %u positions, %u rays", SHARDS, per, total);
    for (uint32_t g = 0; g < SHARDS; ++g)
        REQUIRE(t.runStart[g + 1] - t.runStart[g] <= (uint64_t)((nonEmpty + SHARDS - 1u) / SHARDS) * cellMax * batch, "run %u is %u long", g, t.runStart[g + 1] - t.runStart[g]);
    // a list of whole cells of one size whose number is a multiple of 8: the runs ARE the shards
    bool uniform = nonEmpty == nCells && nCells % SHARDS == 0u && total % (64u * SHARDS) == 0u;
    for (uint32_t k = 0; k < nCells; ++k)
        uniform = uniform && cellValid[k] == cellMax;
    for (uint32_t g = 0; uniform && g <= SHARDS; ++g)
        REQUIRE(t.runStart[g] == g * per, "uniform cells: run %u starts at %u, shard at %u", g, t.runStart[g], g * per);

    printf("OK total=%u per=%u region=%u blocks=%u partial=%u empty=%u cells=%u uniform=%d runs=%s\n", total, per, region, blocks, partial, empty, nonEmpty, uniform ? 1 : 0, runs.c_str());
    return 0;
}
