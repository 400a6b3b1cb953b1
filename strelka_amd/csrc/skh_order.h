// skh_order.h -- where a path's camera ray goes in the FIRST ray queue of a pass: the two tables k_raygen adds up.  No HIP in here
// (tests/cpp/queue_order_main.cpp runs it on the host; tests/test_queue_order_cpu.py holds it to its properties).
//
// k_raygen writes the ray of (unit u, sub-frame s, rank r among the unit's valid slots) to queue position
//     qBase[u] + s * subStride[u] + r
// A UNIT is what one table entry stands for: a 512-slot raygen block, or -- when a block is split -- one of its eight 64-slot chunks (a wave).
// Nothing else depends on the position: the path index, the path state and the accumulation order stay with (sub-frame, slot), and the queue is
// cut into SKH_SHARDS equal runs of per_shard() positions whatever the order (shard = position / per).
//
//   slot_order   the slot order, sub-frame after sub-frame: qBase = exclusive prefix of the valid counts, subStride = valid slots per sub-frame.
//   cell_order   a CELL is `cellUnits` consecutive units.  All `batch` sub-frames of a cell lie back to back (subStride = the cell's valid count), so the
//                samples of a pixel are traced together and find each other's nodes, triangles and shading records in the L2.  The cells that hold a
//                valid slot are numbered along a Morton curve over their first pixel (any tile list has one), and dealt round-robin into `shards`
//                runs that follow each other in the queue: run g holds curve positions g, g + shards, g + 2 shards, ...  The runs come out within a
//                cell or two of the equal cuts, so every shard holds cells from all over the image and the shards work on neighbouring cells at the
//                same time -- no shard owns a band of the image.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace skh_order
{
constexpr uint32_t kNoCell = 0xffffffffu;

struct Tables
{
    std::vector<uint32_t> qBase, subStride; // per unit
    uint32_t validPerSub = 0;               // valid slots of one sub-frame; the queue holds validPerSub * batch rays
    // cell_order only: per cell its number along the curve (kNoCell: no valid slot in it), and where each run starts in the queue (runStart[shards] = total)
    std::vector<uint32_t> curvePos, runStart;
};

// the bits of x at the even positions (Morton order inside a tile: slot m of a tile is pixel (even_bits(m), even_bits(m >> 1)))
inline uint32_t even_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x ^ (x >> 1)) & 0x33333333u;
    x = (x ^ (x >> 2)) & 0x0f0f0f0fu;
    x = (x ^ (x >> 4)) & 0x00ff00ffu;
    x = (x ^ (x >> 8)) & 0x0000ffffu;
    return x;
}

inline uint64_t spread_bits(uint32_t x)
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}
inline uint64_t morton_key(uint32_t x, uint32_t y)
{
    return spread_bits(x) | (spread_bits(y) << 1);
}

// positions per shard: the cut k_raygen makes (whole waves; the last shard is shorter)
inline uint32_t per_shard(uint32_t total, uint32_t shards)
{
    return (((total + shards - 1u) / shards) + 63u) & ~63u;
}

inline void slot_order(const uint32_t* valid, uint32_t nUnits, Tables& t)
{
    t.qBase.assign(std::max(1u, nUnits), 0u);
    t.curvePos.clear(), t.runStart.clear();
    uint32_t total = 0;
    for (uint32_t u = 0; u < nUnits; ++u)
    {
        t.qBase[u] = total;
        total += valid[u];
    }
    t.validPerSub = total;
    t.subStride.assign(std::max(1u, nUnits), total);
}

// originXY: the first pixel of every unit (x, y); valid: its valid slots (0 for a unit outside the image or in a frozen tile)
inline void cell_order(const uint32_t* valid, const uint32_t* originXY, uint32_t nUnits, uint32_t batch, uint32_t cellUnits, uint32_t shards, Tables& t)
{
    cellUnits = std::max(1u, cellUnits), shards = std::max(1u, shards);
    const uint32_t nCells = (nUnits + cellUnits - 1u) / cellUnits;
    std::vector<uint32_t> cellValid(nCells, 0u);
    for (uint32_t u = 0; u < nUnits; ++u)
        cellValid[u / cellUnits] += valid[u];
    // the curve: cells with a valid slot, by the Morton key of their first pixel (ties -- a tile listed twice -- by index)
    std::vector<uint32_t> curve;
    for (uint32_t k = 0; k < nCells; ++k)
        if (cellValid[k])
            curve.push_back(k);
    std::stable_sort(curve.begin(), curve.end(), [&](uint32_t a, uint32_t b) {
        return morton_key(originXY[2 * (size_t)a * cellUnits], originXY[2 * (size_t)a * cellUnits + 1]) < morton_key(originXY[2 * (size_t)b * cellUnits], originXY[2 * (size_t)b * cellUnits + 1]);
    });
    t.curvePos.assign(nCells, kNoCell);
    for (uint32_t i = 0; i < (uint32_t)curve.size(); ++i)
        t.curvePos[curve[i]] = i;
    // the queue: run 0's cells in curve order, then run 1's, ...; a cell takes batch * cellValid positions
    std::vector<uint32_t> cellBase(nCells, 0u);
    t.runStart.assign(shards + 1u, 0u);
    uint32_t pos = 0, perSub = 0;
    for (uint32_t g = 0; g < shards; ++g)
    {
        t.runStart[g] = pos;
        for (size_t i = g; i < curve.size(); i += shards)
        {
            cellBase[curve[i]] = pos;
            pos += cellValid[curve[i]] * batch;
            perSub += cellValid[curve[i]];
        }
    }
    t.runStart[shards] = pos;
    t.validPerSub = perSub;
    t.qBase.assign(std::max(1u, nUnits), 0u);
    t.subStride.assign(std::max(1u, nUnits), 0u);
    for (uint32_t k = 0; k < nCells; ++k)
    {
        uint32_t inCell = 0;
        for (uint32_t u = k * cellUnits; u < std::min(nUnits, (k + 1u) * cellUnits); ++u)
        {
            t.qBase[u] = cellBase[k] + inCell;
            t.subStride[u] = cellValid[k];
            inCell += valid[u];
        }
    }
}
} // namespace skh_order
