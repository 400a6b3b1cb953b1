// skh_accel.inc -- host side of the acceleration structures: the LBVH builder, the host TLAS, skh_build_accel and the in-place updates.
// Included by strelka_hip.hip (one translation unit); needs skh_host.h, spec_drop and build_shading_tables above it.

// world->object of an affine 3x4: the 3x3 by the fp64 adjugate, one rounding to fp32; the fourth column carries the object-to-world
// TRANSLATION itself (points go through xform_point_rel: R^-1 (p - T); DESIGN.md "instance transforms")
static bool invert_affine(const float* m, float* out)
{
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double tx = m[3], ty = m[7], tz = m[11];
    const double A = e * i - f * h, B = c * h - b * i, C = b * f - c * e;
    const double D = f * g - d * i, E = a * i - c * g, F = c * d - a * f;
    const double G = d * h - e * g, H = b * g - a * h, I = a * e - b * d;
    const double det = a * A + b * D + c * G;
    const double r = 1.0 / det;
    const double i00 = A * r, i01 = B * r, i02 = C * r, i10 = D * r, i11 = E * r, i12 = F * r, i20 = G * r, i21 = H * r, i22 = I * r;
#if SKH_ENTRY_REL
    out[0] = (float)i00, out[1] = (float)i01, out[2] = (float)i02, out[3] = (float)tx;
    out[4] = (float)i10, out[5] = (float)i11, out[6] = (float)i12, out[7] = (float)ty;
    out[8] = (float)i20, out[9] = (float)i21, out[10] = (float)i22, out[11] = (float)tz;
#else
    out[0] = (float)i00, out[1] = (float)i01, out[2] = (float)i02, out[3] = (float)(-(i00 * tx + i01 * ty + i02 * tz));
    out[4] = (float)i10, out[5] = (float)i11, out[6] = (float)i12, out[7] = (float)(-(i10 * tx + i11 * ty + i12 * tz));
    out[8] = (float)i20, out[9] = (float)i21, out[10] = (float)i22, out[11] = (float)(-(i20 * tx + i21 * ty + i22 * tz));
#endif
    bool finite = true;
    for (int k = 0; k < 12; ++k)
        finite = finite && std::isfinite(out[k]);
    return finite;
}

// ---------------------------------------------------------------------------------------------------------------
// generic LBVH build over n primitives with boxes + group ids already on the device: lbvh_build is a driver over the stages below
// ---------------------------------------------------------------------------------------------------------------
struct LbvhOut
{
    DevBuf nodes, sortedVals, groupRoot, groupBounds;
    std::vector<int> hostGroupRoot;
    uint32_t numNodes = 0;
    std::vector<uint32_t> levelStart; // the collapse's node slots per level: level L = [levelStart[L], levelStart[L + 1]) -- every child node lies in a later level (skh_refit_accel)
    uint32_t numSlots = 0; // entries of sortedVals: n, or more when the leaves were laid out by 128-byte line (0xffffffff = padding slot)
    // the reinsertion pass (skh_bvh.h k_ri_*), when it ran: rounds done, moves applied, sum of the internal nodes' box areas before / after, time
    uint32_t riRounds = 0, riMoves = 0, riMinSize = 0;
    double riCostBefore = 0.0, riCostAfter = 0.0, riMs = 0.0;
};

// What lbvh_build's stages hand each other.  Each struct is one lifetime: its buffers are freed where the struct goes out of scope.
struct LbvhArgs
{
    uint32_t n, nGroups;
    const std::vector<uint32_t>& groupCount;
    const float4 *boxLo, *boxHi;
    const uint32_t* grp;
    int leafMax;
    int search; // PLOC search radius: 0 triangles, 1 TLAS, 2 curve sub-segments
    uint32_t riRounds, riMinSize;
    std::vector<uint32_t> groupFirst; // first primitive of each group in the sorted order
};
struct LbvhSorted // the sort's buffers: the keys are read by both tree builders (freed when the build ends)
{
    DevBuf gbU, keysA, keysB, valsB, hist, histSums;
    const uint64_t* keys = nullptr; // sorted: keysA or keysB
    uint32_t keyShift = 0;
};
struct LbvhBinary // the binary tree either builder leaves for the collapse (freed when the build ends)
{
    DevBuf childL, childR, parent, rangeF, rangeL, flags, nodeLo, nodeHi, gFirst, gCount;
};
struct LbvhWork // the collapse's queues and orders (freed before the build's last synchronisation)
{
    DevBuf nodeSize, leafOrder, vals2, q[2], ctr;
};

// group bounds, Morton keys, radix sort over the Morton bits + the group bits: out.sortedVals = primitives in key order
static skh_status lbvh_sort(skh_context* c, const LbvhArgs& a, LbvhOut& out, LbvhSorted& so)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, nGroups = a.nGroups;
    SKH_CHECK(dev_alloc(c, so.gbU, sizeof(uint32_t) * 6 * (size_t)nGroups));
    SKH_CHECK(dev_alloc(c, so.keysA, sizeof(uint64_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, so.keysB, sizeof(uint64_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, so.valsB, sizeof(uint32_t) * (size_t)n));
    const uint32_t rsBlocks = (n + SKH_RS_THREADS * SKH_RS_ITEMS - 1) / (SKH_RS_THREADS * SKH_RS_ITEMS);
    SKH_CHECK(dev_alloc(c, so.hist, sizeof(uint32_t) * 256 * (size_t)rsBlocks));
    // the digit histograms (256 x blocks words: 1.4 M for 23 M keys) are scanned by many workgroups -- blocks of 4096, a one-workgroup scan of
    // the block sums, an add pass -- not by ONE workgroup walking the whole array (round 3: up to 2.5 ms per sort pass, eight passes)
    const uint32_t histWords = 256u * rsBlocks, histBlocks = (histWords + SKH_SCAN_BLOCK * SKH_SCAN_ITEMS - 1) / (SKH_SCAN_BLOCK * SKH_SCAN_ITEMS);
    SKH_CHECK(dev_alloc(c, so.histSums, sizeof(uint32_t) * (size_t)(histBlocks + 1)));
    const uint32_t B = 256, G1 = (n + B - 1) / B;
    k_init_group_bounds<<<(nGroups * 6 + B - 1) / B, B, 0, st>>>(so.gbU.as<uint32_t>(), nGroups);
    k_group_bounds<<<(G1 + SKH_GB_RUN - 1) / SKH_GB_RUN, B, 0, st>>>(a.boxLo, a.boxHi, a.grp, n, so.gbU.as<uint32_t>()); // (a wave walks SKH_GB_RUN rows of 64)
    k_decode_group_bounds<<<(nGroups * 6 + B - 1) / B, B, 0, st>>>(so.gbU.as<uint32_t>(), out.groupBounds.as<float>(), nGroups);
    uint32_t* valsA = out.sortedVals.as<uint32_t>();
    // sort key: group id above a Morton code of `morton_bits` (10) bits per axis -- fewer when the group ids need the room
    uint32_t gbits = 0;
    while ((1ull << gbits) < (unsigned long long)nGroups)
        ++gbits;
    const uint32_t mb = std::min<uint32_t>(c->opt.mortonBits, (64u - gbits) / 3u);
    so.keyShift = 3u * mb;
    k_morton<<<G1, B, 0, st>>>(a.boxLo, a.boxHi, a.grp, out.groupBounds.as<float>(), n, mb, so.keysA.as<uint64_t>(), valsA);
    uint64_t* kin = so.keysA.as<uint64_t>();
    uint64_t* kout = so.keysB.as<uint64_t>();
    uint32_t* vin = valsA;
    uint32_t* vout = so.valsB.as<uint32_t>();
    for (uint32_t shift = 0; shift < so.keyShift + gbits; shift += 8)
    {
        k_rs_hist<<<rsBlocks, SKH_RS_THREADS, 0, st>>>(kin, n, shift, so.hist.as<uint32_t>(), rsBlocks, nullptr);
        if (histBlocks > 1)
        {
            k_scan_block<<<histBlocks, SKH_SCAN_BLOCK, 0, st>>>(so.hist.as<uint32_t>(), histWords, so.histSums.as<uint32_t>());
            k_rs_scan<<<1, 1024, 0, st>>>(so.histSums.as<uint32_t>(), histBlocks);
            k_scan_add<<<histBlocks, SKH_SCAN_BLOCK, 0, st>>>(so.hist.as<uint32_t>(), histWords, so.histSums.as<uint32_t>());
        }
        else
            k_rs_scan<<<1, 1024, 0, st>>>(so.hist.as<uint32_t>(), histWords);
        k_rs_scatter<<<rsBlocks, SKH_RS_THREADS, 0, st>>>(kin, vin, kout, vout, n, shift, so.hist.as<uint32_t>(), rsBlocks, nullptr);
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    if (vin != valsA) // odd number of passes: bring the values home
        SKH_TRY(c, hipMemcpyAsync(valsA, vin, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    so.keys = kin;
    return SKH_OK;
}

// agglomerative clustering over the Morton order; its own buffers die here.  Returns the node ids it handed out.
static skh_status lbvh_ploc(skh_context* c, const LbvhArgs& a, const LbvhOut& out, const LbvhSorted& so, LbvhBinary& bt, LbvhWork& wk, uint32_t& nInternal)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, B = 256, G1 = (n + B - 1) / B;
    DevBuf cLo[2], cHi[2], nn, pflags, ppos, scanSums;
    for (int k = 0; k < 2; ++k)
    {
        SKH_CHECK(dev_alloc(c, cLo[k], sizeof(float4) * (size_t)n));
        SKH_CHECK(dev_alloc(c, cHi[k], sizeof(float4) * (size_t)n));
    }
    SKH_CHECK(dev_alloc(c, nn, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, pflags, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, ppos, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, scanSums, sizeof(uint32_t) * (size_t)(n / (SKH_SCAN_BLOCK * SKH_SCAN_ITEMS) + 2)));
    uint32_t nonEmpty = 0;
    for (uint32_t g = 0; g < a.nGroups; ++g)
        nonEmpty += a.groupCount[g] ? 1u : 0u;
    uint32_t hc[4] = { 0, 0, 0, 0 }; // [2] PLOC node counter, [3] surviving cluster count
    SKH_TRY(c, hipMemcpyAsync(wk.ctr.p, hc, sizeof(hc), hipMemcpyHostToDevice, st));
    if (a.riRounds)
    {
        SKH_CHECK(dev_alloc(c, bt.parent, sizeof(int) * 2 * (size_t)n));
        SKH_TRY(c, hipMemsetAsync(bt.parent.p, 0xff, sizeof(int) * 2 * (size_t)n, st)); // -1: roots (and the ids PLOC never hands out) have no parent
    }
    k_ploc_init<<<G1, B, 0, st>>>(out.sortedVals.as<uint32_t>(), so.keys, a.boxLo, a.boxHi, n, cLo[0].as<float4>(), cHi[0].as<float4>(),
                                  bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), so.keyShift);
    uint32_t m = n;
    int cur = 0;
    bool paired = SKH_PLOC_PAIRED_FIRST != 0;
    int slow = 0;
    // one round: name a partner per cluster, merge the pairs that name each other, compact.  `adjacent` < 0: the cost search (k_ploc_nn); 0 / 1: the
    // round of last resort with that parity (k_ploc_nn_adjacent).  -> hc[3] = clusters left
    auto round = [&](int adjacent) -> skh_status {
        const uint32_t gm = (m + SKH_PLOC_BLOCK - 1) / SKH_PLOC_BLOCK;
        if (adjacent >= 0)
            k_ploc_nn_adjacent<<<(m + B - 1) / B, B, 0, st>>>(cHi[cur].as<float4>(), m, (uint32_t)adjacent, nn.as<uint32_t>());
        else
        {
            // the top of a triangle tree -- the levels every ray walks -- is clustered with the wide search of the TLAS builder (option ploc_top; few clusters left: cheap)
            const int radius = a.search == 1 ? SKH_PLOC_RADIUS_TLAS : a.search == 2 ? SKH_PLOC_RADIUS_SEGS : m <= c->opt.plocTop ? SKH_PLOC_RADIUS_TLAS : SKH_PLOC_RADIUS;
            auto search = [&](auto r) {
                constexpr int R = decltype(r)::value;
                if (paired)
                    k_ploc_nn<R, true><<<gm, SKH_PLOC_BLOCK, 0, st>>>(cLo[cur].as<float4>(), cHi[cur].as<float4>(), m, nn.as<uint32_t>());
                else
                    k_ploc_nn<R, false><<<gm, SKH_PLOC_BLOCK, 0, st>>>(cLo[cur].as<float4>(), cHi[cur].as<float4>(), m, nn.as<uint32_t>());
            };
            if (radius == SKH_PLOC_RADIUS_TLAS)
                search(std::integral_constant<int, SKH_PLOC_RADIUS_TLAS>());
            else if (radius == SKH_PLOC_RADIUS_SEGS)
                search(std::integral_constant<int, SKH_PLOC_RADIUS_SEGS>());
            else
                search(std::integral_constant<int, SKH_PLOC_RADIUS>());
        }
        k_ploc_merge<<<(m + B - 1) / B, B, 0, st>>>(cLo[cur].as<float4>(), cHi[cur].as<float4>(), nn.as<uint32_t>(), m, (int)n,
                                                    bt.childL.as<int>(), bt.childR.as<int>(), wk.nodeSize.as<int>(), bt.nodeLo.as<float4>(),
                                                    bt.nodeHi.as<float4>(), wk.ctr.as<uint32_t>() + 2, pflags.as<uint32_t>(), a.riRounds ? bt.parent.as<int>() : nullptr);
        SKH_TRY(c, hipMemcpyAsync(ppos.p, pflags.p, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToDevice, st));
        {
            const uint32_t sb = (m + SKH_SCAN_BLOCK * SKH_SCAN_ITEMS - 1) / (SKH_SCAN_BLOCK * SKH_SCAN_ITEMS);
            k_scan_block<<<sb, SKH_SCAN_BLOCK, 0, st>>>(ppos.as<uint32_t>(), m, scanSums.as<uint32_t>());
            k_rs_scan<<<1, 1024, 0, st>>>(scanSums.as<uint32_t>(), sb);
            k_scan_add<<<sb, SKH_SCAN_BLOCK, 0, st>>>(ppos.as<uint32_t>(), m, scanSums.as<uint32_t>());
        }
        k_ploc_compact<<<(m + B - 1) / B, B, 0, st>>>(cLo[cur].as<float4>(), cHi[cur].as<float4>(), pflags.as<uint32_t>(),
                                                      ppos.as<uint32_t>(), m, cLo[cur ^ 1].as<float4>(), cHi[cur ^ 1].as<float4>(),
                                                      wk.ctr.as<uint32_t>() + 3);
        SKH_TRY(c, hipMemcpyAsync(hc, wk.ctr.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        return SKH_OK;
    };
    for (int iter = 0; m > nonEmpty && iter < SKH_PLOC_MAX_ROUNDS; ++iter)
    {
        SKH_CHECK(round(-1));
        if (hc[3] >= m) // no progress: cannot happen (a mutually-nearest pair always exists), but never spin
            break;
        // Two rounds in a row that each did less than a sixteenth of the merges still to do (m - nonEmpty: a finished group's cluster does not count): tied
        // boxes chain under "the lowest index wins" (k_ploc_nn), one merge a round.  The rest of this build breaks ties the PAIRED way.
        slow = (uint64_t)(m - hc[3]) * 16u < m - nonEmpty ? slow + 1 : 0;
        if (slow >= 2)
            paired = true;
        m = hc[3];
        cur ^= 1;
    }
    // Every primitive handed in is in the hierarchy: whatever the search left unmerged -- it ran out of rounds, or left its loop on a round without a merge -- is paired off by position (skh_bvh.h
    // k_ploc_nn_adjacent).  Two rounds of alternating parity in a row without a merge cannot happen while a group holds two clusters.
    for (int iter = 0, idle = 0; m > nonEmpty && idle < 2 && iter < 128; ++iter)
    {
        SKH_CHECK(round(iter & 1));
        idle = hc[3] >= m ? idle + 1 : 0;
        if (hc[3] < m)
        {
            m = hc[3];
            cur ^= 1;
        }
    }
    if (m != nonEmpty) // k_ploc_roots writes one root per cluster: with more clusters than groups all but one of a group's subtrees would be lost
    {
        c->dev.err = "lbvh_build: the clustering ended with " + std::to_string(m) + " clusters for " + std::to_string(nonEmpty) + " non-empty groups";
        return SKH_FAIL;
    }
    k_ploc_roots<<<(m + B - 1) / B, B, 0, st>>>(cLo[cur].as<float4>(), cHi[cur].as<float4>(), m, out.groupRoot.as<int>());
    nInternal = hc[2];
    return SKH_OK;
}

// refit of the paths the round's moves stamped, one tree level per launch (rflags = stamped children still to come; lists ping-pong in `refitList`)
static skh_status lbvh_reinsert_refit(skh_context* c, uint32_t n, uint32_t round, LbvhBinary& bt, LbvhWork& wk, DevBuf& stamp, DevBuf& rflags, DevBuf& refitList,
                                      DevBuf& refitCount)
{
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256;
    uint32_t* lv = refitCount.as<uint32_t>();
    SKH_TRY(c, hipMemsetAsync(lv, 0, sizeof(uint32_t) * SKH_RI_MAX_LEVELS, st));
    uint32_t* lists[2] = { refitList.as<uint32_t>(), refitList.as<uint32_t>() + n };
    k_ri_pending<<<(n + B - 1) / B, B, 0, st>>>(bt.childL.as<int>(), bt.childR.as<int>(), stamp.as<uint32_t>(), round, (int)n, rflags.as<uint32_t>(), lists[0], lv);
    // (the per-level counters are a RING: a binary tree deeper than SKH_RI_MAX_LEVELS -- nested "onion" geometry, chains the moves themselves
    // grow -- wraps around it, each reused counter zeroed before its level runs, instead of failing the whole build for an optional
    // pass: ADVICE r5.  A tree has at most n levels.)
    for (uint32_t k = 0; k < n; ++k)
    {
        const uint32_t ci = k % SKH_RI_MAX_LEVELS, cn = (k + 1u) % SKH_RI_MAX_LEVELS;
        if (k + 1u >= SKH_RI_MAX_LEVELS)
            SKH_TRY(c, hipMemsetAsync(lv + cn, 0, sizeof(uint32_t), st));
        k_ri_refit_level<<<256, B, 0, st>>>(lists[k & 1], lv + ci, lists[(k + 1) & 1], lv + cn, bt.parent.as<int>(), bt.childL.as<int>(), bt.childR.as<int>(),
                                            rflags.as<uint32_t>(), bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), wk.nodeSize.as<int>(), (int)n);
        if ((k & 15u) == 15u || k + 1u == n) // (and after the last level: a tree of fewer than 16 levels has no sixteenth)
        {
            uint32_t next = 0;
            SKH_TRY(c, hipMemcpyAsync(&next, lv + cn, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            SKH_TRY(c, hipStreamSynchronize(st));
            if (next == 0)
                return SKH_OK;
        }
    }
    c->dev.err = "lbvh_build: the reinsertion pass's refit did not finish within n levels (a cycle in the tree?)";
    return SKH_FAIL;
}

// parallel reinsertion over the binary tree (skh_bvh.h): rounds of search / claim / own / check / apply / refit; its twelve buffers die here
static skh_status lbvh_reinsert(skh_context* c, const LbvhArgs& a, uint32_t nInternal, LbvhBinary& bt, LbvhWork& wk, LbvhOut& out)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, B = 256;
    DevBuf moves, lock, moving, win, rflags, cost, cand, stamp, refitList, refitCount, activeA, activeB;
    const size_t N2 = 2 * (size_t)n;
    SKH_CHECK(dev_alloc(c, moves, sizeof(int4) * N2));
    SKH_CHECK(dev_alloc(c, lock, sizeof(unsigned long long) * N2));
    SKH_CHECK(dev_alloc(c, moving, sizeof(unsigned long long) * N2));
    SKH_CHECK(dev_alloc(c, win, N2));
    SKH_CHECK(dev_alloc(c, rflags, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, cost, sizeof(double) * 2 + sizeof(uint32_t) * 2));
    SKH_CHECK(dev_alloc(c, cand, sizeof(uint32_t) * N2));
    SKH_CHECK(dev_alloc(c, stamp, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, refitList, sizeof(uint32_t) * 2 * (size_t)n));
    SKH_CHECK(dev_alloc(c, refitCount, sizeof(uint32_t) * SKH_RI_MAX_LEVELS));
    SKH_CHECK(dev_alloc(c, activeA, N2));
    SKH_CHECK(dev_alloc(c, activeB, N2));
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t GN = (uint32_t)((N2 + B - 1) / B);
    double* dCost = cost.as<double>();
    uint32_t* dWin = reinterpret_cast<uint32_t*>(dCost + 2); // [0] moves applied this round, [1] candidates
    SKH_TRY(c, hipMemsetAsync(cost.p, 0, sizeof(double) * 2 + sizeof(uint32_t) * 2, st));
    SKH_TRY(c, hipMemsetAsync(stamp.p, 0, sizeof(uint32_t) * (size_t)n, st));
    k_ri_cost<<<1024, B, 0, st>>>(bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), (int)nInternal, dCost);
    out.riMinSize = a.riMinSize;
    uint32_t nCandHost = (uint32_t)N2; // (the list kernels are sized by the round's candidate count, read back below)
    for (uint32_t r = 0; r < a.riRounds; ++r)
    {
        SKH_TRY(c, hipMemsetAsync(lock.p, 0, sizeof(unsigned long long) * N2, st));
        SKH_TRY(c, hipMemsetAsync(moving.p, 0, sizeof(unsigned long long) * N2, st));
        SKH_TRY(c, hipMemsetAsync(dWin, 0, sizeof(uint32_t) * 2, st));
        // every third round searches from every node; the rounds between from last round's candidates and the nodes next to its moves only
        uint8_t* activeCur = (r & 1u) ? activeB.as<uint8_t>() : activeA.as<uint8_t>();
        uint8_t* activeNext = (r & 1u) ? activeA.as<uint8_t>() : activeB.as<uint8_t>();
        SKH_TRY(c, hipMemsetAsync(activeNext, 0, N2, st));
        k_ri_search<<<GN, B, 0, st>>>(bt.childL.as<int>(), bt.childR.as<int>(), bt.parent.as<int>(), wk.nodeSize.as<int>(), bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), (int)n,
                                      (int)a.riMinSize, (r % 3u) == 0u ? nullptr : activeCur, moves.as<int4>(), cand.as<uint32_t>(), dWin + 1);
        // the list kernels are sized by the candidate count, read back here (one small synchronisation per round; the search is the long kernel)
        SKH_TRY(c, hipMemcpyAsync(&nCandHost, dWin + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        out.riRounds = r + 1;
        if (nCandHost == 0)
            break;
        const uint32_t GC = (nCandHost + B - 1) / B;
        k_ri_claim<<<GC, B, 0, st>>>(moves.as<int4>(), cand.as<uint32_t>(), dWin + 1, bt.childL.as<int>(), bt.childR.as<int>(), bt.parent.as<int>(), lock.as<unsigned long long>(), activeNext);
        k_ri_own<<<GC, B, 0, st>>>(moves.as<int4>(), cand.as<uint32_t>(), dWin + 1, bt.childL.as<int>(), bt.childR.as<int>(), bt.parent.as<int>(), lock.as<unsigned long long>(),
                                   moving.as<unsigned long long>());
        k_ri_check<<<GC, B, 0, st>>>(moves.as<int4>(), cand.as<uint32_t>(), dWin + 1, bt.parent.as<int>(), moving.as<unsigned long long>(), win.as<uint8_t>(), dWin);
        k_ri_apply<<<GC, B, 0, st>>>(moves.as<int4>(), cand.as<uint32_t>(), dWin + 1, win.as<uint8_t>(), bt.childL.as<int>(), bt.childR.as<int>(), bt.parent.as<int>());
        k_ri_mark<<<GC, B, 0, st>>>(moves.as<int4>(), cand.as<uint32_t>(), dWin + 1, win.as<uint8_t>(), bt.parent.as<int>(), bt.childL.as<int>(), bt.childR.as<int>(), stamp.as<uint32_t>(), r + 1u, activeNext);
        SKH_CHECK(lbvh_reinsert_refit(c, n, r + 1u, bt, wk, stamp, rflags, refitList, refitCount));
        uint32_t moved = 0;
        SKH_TRY(c, hipMemcpyAsync(&moved, dWin, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        out.riMoves += moved;
        if (moved == 0)
            break;
    }
    double hcost[2] = { 0, 0 };
    k_ri_cost<<<1024, B, 0, st>>>(bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), (int)nInternal, dCost + 1);
    SKH_TRY(c, hipMemcpyAsync(hcost, dCost, sizeof(hcost), hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    out.riCostBefore = hcost[0], out.riCostAfter = hcost[1];
    out.riMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SKH_OK;
}

// Karras radix tree over the sorted keys
static skh_status lbvh_karras(skh_context* c, const LbvhArgs& a, const LbvhOut& out, const LbvhSorted& so, LbvhBinary& bt, LbvhWork& wk)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, B = 256, G1 = (n + B - 1) / B;
    SKH_CHECK(dev_alloc(c, bt.parent, sizeof(int) * 2 * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.rangeF, sizeof(int) * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.rangeL, sizeof(int) * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.flags, sizeof(uint32_t) * (size_t)n));
    SKH_TRY(c, hipMemsetAsync(bt.flags.p, 0, sizeof(uint32_t) * (size_t)n, st));
    k_karras<<<(n - 1 + B - 1) / B, B, 0, st>>>(so.keys, (int)n, bt.childL.as<int>(), bt.childR.as<int>(), bt.parent.as<int>(),
                                               bt.rangeF.as<int>(), bt.rangeL.as<int>());
    k_refit<<<G1, B, 0, st>>>(out.sortedVals.as<uint32_t>(), a.boxLo, a.boxHi, bt.parent.as<int>(), bt.childL.as<int>(), bt.childR.as<int>(), bt.flags.as<uint32_t>(),
                              bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), (int)n);
    k_sizes_from_ranges<<<(n - 1 + B - 1) / B, B, 0, st>>>(bt.rangeF.as<int>(), bt.rangeL.as<int>(), (int)n, wk.nodeSize.as<int>());
    k_group_roots<<<(n - 1 + B - 1) / B, B, 0, st>>>(bt.rangeF.as<int>(), bt.rangeL.as<int>(), so.keys, bt.gFirst.as<uint32_t>(),
                                                    bt.gCount.as<uint32_t>(), (int)n, a.leafMax, so.keyShift, out.groupRoot.as<int>());
    return SKH_OK;
}

// the group roots come back as BINARY node ids; they seed the level-by-level collapse into 4-wide nodes, which leaves the primitives in leaf order
static skh_status lbvh_collapse(skh_context* c, const LbvhArgs& a, const std::vector<int>& preset /* leaf refs of groups with <= leafMax primitives, INVALID otherwise */,
                                LbvhBinary& bt, LbvhWork& wk, LbvhOut& out)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, nGroups = a.nGroups, B = 256, G1 = (n + B - 1) / B;
    uint32_t* valsA = out.sortedVals.as<uint32_t>();
    SKH_TRY(c, hipMemcpyAsync(out.hostGroupRoot.data(), out.groupRoot.p, sizeof(int) * nGroups, hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    std::vector<CollapseItem> seed;
    for (uint32_t g = 0; g < nGroups; ++g)
    {
        if (a.groupCount[g] <= (uint32_t)a.leafMax)
            out.hostGroupRoot[g] = preset[g]; // whole group is one leaf (or empty)
        else
        {
            seed.push_back(CollapseItem{ out.hostGroupRoot[g], (int)seed.size(), (int)a.groupFirst[g], 0 });
            out.hostGroupRoot[g] = (int)seed.size() - 1;
        }
    }
    uint32_t cnt = (uint32_t)seed.size();
    uint32_t hctr[2] = { cnt, 0 }; // [0] next free output slot, [1] next-level queue length
    if (cnt)
        SKH_TRY(c, hipMemcpyAsync(wk.q[0].p, seed.data(), sizeof(CollapseItem) * cnt, hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipMemcpyAsync(wk.ctr.p, hctr, sizeof(hctr), hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipMemcpyAsync(out.groupRoot.p, out.hostGroupRoot.data(), sizeof(int) * nGroups, hipMemcpyHostToDevice, st));
    k_iota<<<G1, B, 0, st>>>(wk.leafOrder.as<uint32_t>(), n);
    int cur = 0;
    out.levelStart.assign(1, 0u);
    out.levelStart.push_back(cnt); // (level 0 = the groups' roots)
    while (cnt > 0)
    {
        k_collapse<<<(cnt + B - 1) / B, B, 0, st>>>(wk.q[cur].as<CollapseItem>(), cnt, bt.childL.as<int>(), bt.childR.as<int>(), wk.nodeSize.as<int>(),
                                                       bt.nodeLo.as<float4>(), bt.nodeHi.as<float4>(), (int)n, a.leafMax, out.nodes.p, wk.ctr.as<uint32_t>(),
                                                       wk.q[cur ^ 1].as<CollapseItem>(), wk.ctr.as<uint32_t>() + 1, wk.leafOrder.as<uint32_t>(), a.search == 0 ? c->opt.splitPairs * 0.1f : 0.0f);
        SKH_TRY(c, hipMemcpyAsync(hctr, wk.ctr.p, sizeof(hctr), hipMemcpyDeviceToHost, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        cnt = hctr[1];
        if (cnt)
            out.levelStart.push_back(hctr[0]); // (the next level's nodes took the slots up to here)
        const uint32_t zero = 0;
        SKH_TRY(c, hipMemcpyAsync(wk.ctr.as<uint32_t>() + 1, &zero, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        cur ^= 1;
    }
    // primitives into final leaf order
    k_permute_u32<<<G1, B, 0, st>>>(valsA, wk.leafOrder.as<uint32_t>(), n, wk.vals2.as<uint32_t>());
    SKH_TRY(c, hipMemcpyAsync(valsA, wk.vals2.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    out.numNodes = hctr[0];
    return SKH_OK;
}

// leaves by 128-byte line (skh_bvh.h: k_leaf_place): padding slots in front of the leaves that would straddle; its buffers (and the unpadded order) die here
static skh_status lbvh_leaf_lines(skh_context* c, const LbvhArgs& a, uint32_t lineRecBytes, LbvhOut& out)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, nGroups = a.nGroups, B = 256, G1 = (n + B - 1) / B;
    DevBuf leafCnt, chunk, remap, sums, vals3;
    const uint32_t nCh = (n + SKH_LEAF_CHUNK - 1u) / SKH_LEAF_CHUNK;
    const uint32_t sb = (nCh + SKH_SCAN_BLOCK * SKH_SCAN_ITEMS - 1) / (SKH_SCAN_BLOCK * SKH_SCAN_ITEMS);
    SKH_CHECK(dev_alloc(c, leafCnt, (size_t)n));
    SKH_CHECK(dev_alloc(c, chunk, sizeof(uint32_t) * (size_t)nCh));
    SKH_CHECK(dev_alloc(c, remap, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, sums, sizeof(uint32_t) * ((size_t)sb + 2)));
    int* nodeRefs = reinterpret_cast<int*>(out.nodes.p) + 12; // Node4::child
    const uint32_t nRefs = out.numNodes * 4u;
    SKH_TRY(c, hipMemsetAsync(leafCnt.p, 0, (size_t)n, st));
    if (nRefs)
        k_leaf_mark<<<(nRefs + B - 1) / B, B, 0, st>>>(nodeRefs, nRefs, 16u, 4u, leafCnt.as<uint8_t>());
    k_leaf_mark<<<(nGroups + B - 1) / B, B, 0, st>>>(out.groupRoot.as<int>(), nGroups, 1u, 1u, leafCnt.as<uint8_t>());
    k_leaf_place<<<(nCh + B - 1) / B, B, 0, st>>>(leafCnt.as<uint8_t>(), n, lineRecBytes, nullptr, chunk.as<uint32_t>(), nullptr);
    uint32_t lastLen = 0, lastBase = 0;
    SKH_TRY(c, hipMemcpyAsync(&lastLen, chunk.as<uint32_t>() + (nCh - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    k_scan_block<<<sb, SKH_SCAN_BLOCK, 0, st>>>(chunk.as<uint32_t>(), nCh, sums.as<uint32_t>());
    k_rs_scan<<<1, 1024, 0, st>>>(sums.as<uint32_t>(), sb);
    k_scan_add<<<sb, SKH_SCAN_BLOCK, 0, st>>>(chunk.as<uint32_t>(), nCh, sums.as<uint32_t>());
    SKH_TRY(c, hipMemcpyAsync(&lastBase, chunk.as<uint32_t>() + (nCh - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    const uint64_t total = (uint64_t)lastBase + lastLen;
    if (total >= (1ull << 28))
    {
        c->dev.err = "lbvh_build: more than 2^28 leaf slots";
        return SKH_INVALID_ARGUMENT;
    }
    SKH_CHECK(dev_alloc(c, vals3, sizeof(uint32_t) * (size_t)std::max<uint64_t>(1, total)));
    k_leaf_place<<<(nCh + B - 1) / B, B, 0, st>>>(leafCnt.as<uint8_t>(), n, lineRecBytes, chunk.as<uint32_t>(), nullptr, remap.as<uint32_t>());
    if (nRefs)
        k_leaf_patch<<<(nRefs + B - 1) / B, B, 0, st>>>(nodeRefs, nRefs, 16u, 4u, remap.as<uint32_t>());
    k_leaf_patch<<<(nGroups + B - 1) / B, B, 0, st>>>(out.groupRoot.as<int>(), nGroups, 1u, 1u, remap.as<uint32_t>());
    SKH_TRY(c, hipMemsetAsync(vals3.p, 0xff, sizeof(uint32_t) * (size_t)total, st));
    k_leaf_scatter<<<G1, B, 0, st>>>(out.sortedVals.as<uint32_t>(), remap.as<uint32_t>(), n, vals3.as<uint32_t>());
    SKH_TRY(c, hipMemcpyAsync(out.hostGroupRoot.data(), out.groupRoot.p, sizeof(int) * nGroups, hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    std::swap(out.sortedVals, vals3); // (the unpadded order is freed with vals3)
    out.numSlots = (uint32_t)total;
    return SKH_OK;
}

// the binary tree (PLOC + reinsertion, or Karras), its collapse and the leaf layout: everything a group of two or more primitives needs
static skh_status lbvh_tree(skh_context* c, const LbvhArgs& a, bool ploc, uint32_t lineRecBytes, const LbvhSorted& so, LbvhBinary& bt, LbvhOut& out)
{
    hipStream_t st = c->dev.stream;
    const uint32_t n = a.n, nGroups = a.nGroups;
    LbvhWork wk;
    SKH_CHECK(dev_alloc(c, bt.childL, sizeof(int) * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.childR, sizeof(int) * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.nodeLo, sizeof(float4) * 2 * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.nodeHi, sizeof(float4) * 2 * (size_t)n));
    SKH_CHECK(dev_alloc(c, bt.gFirst, sizeof(uint32_t) * (size_t)nGroups));
    SKH_CHECK(dev_alloc(c, bt.gCount, sizeof(uint32_t) * (size_t)nGroups));
    SKH_CHECK(dev_alloc(c, wk.nodeSize, sizeof(int) * (size_t)n));
    SKH_CHECK(dev_alloc(c, wk.leafOrder, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, wk.vals2, sizeof(uint32_t) * (size_t)n));
    SKH_CHECK(dev_alloc(c, wk.q[0], sizeof(CollapseItem) * (size_t)n));
    SKH_CHECK(dev_alloc(c, wk.q[1], sizeof(CollapseItem) * (size_t)n));
    SKH_CHECK(dev_alloc(c, wk.ctr, sizeof(uint32_t) * 4));
    SKH_TRY(c, hipMemcpyAsync(bt.gFirst.p, a.groupFirst.data(), sizeof(uint32_t) * nGroups, hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipMemcpyAsync(bt.gCount.p, a.groupCount.data(), sizeof(uint32_t) * nGroups, hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipMemcpyAsync(out.groupRoot.p, out.hostGroupRoot.data(), sizeof(int) * nGroups, hipMemcpyHostToDevice, st));
    const std::vector<int> preset = out.hostGroupRoot;
    if (ploc)
    {
        uint32_t nInternal = 0;
        SKH_CHECK(lbvh_ploc(c, a, out, so, bt, wk, nInternal));
        if (a.riRounds && n >= 8)
            SKH_CHECK(lbvh_reinsert(c, a, nInternal, bt, wk, out));
    }
    else
        SKH_CHECK(lbvh_karras(c, a, out, so, bt, wk));
    SKH_CHECK(lbvh_collapse(c, a, preset, bt, wk, out));
    if (lineRecBytes)
        SKH_CHECK(lbvh_leaf_lines(c, a, lineRecBytes, out));
    return SKH_OK;
}

static skh_status lbvh_build(skh_context* c, uint32_t n, uint32_t nGroups, const std::vector<uint32_t>& groupCount,
                             const float4* dBoxLo, const float4* dBoxHi, const uint32_t* dGrp, int leafMax, bool ploc, LbvhOut& out,
                             int search = 0 /* PLOC search radius: 0 triangles, 1 TLAS, 2 curve sub-segments */, uint32_t lineRecBytes = 0 /* > 0: leaf records of this size, laid out by 128-byte line */,
                             uint32_t riRounds = 0 /* reinsertion rounds after PLOC */, uint32_t riMinSize = 1)
{
    hipStream_t st = c->dev.stream;
    out.numSlots = n;
    SKH_CHECK(dev_alloc(c, out.groupBounds, sizeof(float) * 6 * (size_t)std::max(1u, nGroups)));
    SKH_CHECK(dev_alloc(c, out.groupRoot, sizeof(int) * (size_t)std::max(1u, nGroups)));
    SKH_CHECK(dev_alloc(c, out.nodes, sizeof(Node4) * ((size_t)std::max(1u, n) + 1)));
    SKH_CHECK(dev_alloc(c, out.sortedVals, sizeof(uint32_t) * (size_t)std::max(1u, n)));
    LbvhArgs a{ n, nGroups, groupCount, dBoxLo, dBoxHi, dGrp, leafMax, search, riRounds, riMinSize, std::vector<uint32_t>(nGroups) };
    out.hostGroupRoot.assign(nGroups, SKH_REF_INVALID);
    uint32_t acc = 0;
    for (uint32_t g = 0; g < nGroups; ++g)
    {
        a.groupFirst[g] = acc;
        if (groupCount[g] > 0 && groupCount[g] <= (uint32_t)leafMax)
            out.hostGroupRoot[g] = ~(int)((acc << 3) | (groupCount[g] - 1u));
        acc += groupCount[g];
    }
    if (n == 0 || nGroups == 0)
    {
        if (nGroups)
            SKH_TRY(c, hipMemcpyAsync(out.groupRoot.p, out.hostGroupRoot.data(), sizeof(int) * nGroups, hipMemcpyHostToDevice, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        return SKH_OK;
    }
    LbvhSorted so;
    LbvhBinary bt;
    SKH_CHECK(lbvh_sort(c, a, out, so));
    if (n >= 2)
        SKH_CHECK(lbvh_tree(c, a, ploc, lineRecBytes, so, bt, out));
    else
        SKH_TRY(c, hipMemcpyAsync(out.groupRoot.p, out.hostGroupRoot.data(), sizeof(int) * nGroups, hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    SKH_TRY(c, hipGetLastError());
    return SKH_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------------
// TLAS by full-sweep SAH on the host.  The top level holds a few thousand instance boxes (the reference's IAS,
// OptixRender.cpp:443-495) and every ray walks it, so its quality matters far more than its build time; an exact
// sweep over three axes costs O(n log^2 n) on a few thousand boxes -- well under a millisecond per thousand.
// Invalid (masked-out) instances are left out.  Output: 64-byte nodes + leaf order, same encoding as the GPU LBVH.
// ---------------------------------------------------------------------------------------------------------------
struct HostBox
{
    float lo[3], hi[3];
};
static inline float hb_half_area(const float* lo, const float* hi)
{
    const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    return ex * ey + ey * ez + ez * ex;
}
struct HostBin // internal node of the host-side binary tree
{
    int left, right; // >= 0 HostBin index, < 0 leaf ref
    float lo[3], hi[3];
};
static void hb_box_of_ref(int ref, const std::vector<HostBin>& bin, const std::vector<HostBox>& boxes, float* lo, float* hi)
{
    if (ref >= 0)
    {
        memcpy(lo, bin[ref].lo, sizeof(float) * 3);
        memcpy(hi, bin[ref].hi, sizeof(float) * 3);
    }
    else
    {
        const HostBox& b = boxes[((uint32_t)~ref) >> 3];
        memcpy(lo, b.lo, sizeof(float) * 3);
        memcpy(hi, b.hi, sizeof(float) * 3);
    }
}
static int tlas_sah_build(const std::vector<HostBox>& boxes, const std::vector<uint32_t>& ids, std::vector<Node4>& nodes,
                          std::vector<uint32_t>& order, std::vector<uint32_t>& levelStart /* as LbvhOut::levelStart: the nodes of level L = [levelStart[L], levelStart[L + 1]) */)
{
    const uint32_t n = (uint32_t)ids.size();
    nodes.clear();
    order.clear();
    levelStart.clear();
    if (n == 0)
        return SKH_REF_INVALID;
    order.assign(ids.begin(), ids.end());
    if (n == 1)
        return ~(int)((ids[0] << 3) | 0u);
    std::vector<HostBin> bin;
    struct Task
    {
        uint32_t first, count;
        int parent;
        int side;
    };
    std::vector<Task> stack;
    stack.push_back(Task{ 0, n, -1, 0 });
    std::vector<float> rightArea;
    int rootRef = 0;
    while (!stack.empty())
    {
        const Task t = stack.back();
        stack.pop_back();
        int ref;
        if (t.count == 1)
            ref = ~(int)((order[t.first] << 3) | 0u); // leaf ref carries the INSTANCE ID (one instance per leaf)
        else
        {
            float bestCost = INFINITY;
            int bestAxis = 0;
            uint32_t bestSplit = t.count / 2;
            auto sortAxis = [&](int axis) {
                std::sort(order.begin() + t.first, order.begin() + t.first + t.count, [&](uint32_t a, uint32_t b) {
                    const float ca = boxes[a].lo[axis] + boxes[a].hi[axis], cb = boxes[b].lo[axis] + boxes[b].hi[axis];
                    return ca < cb || (ca == cb && a < b);
                });
            };
            for (int axis = 0; axis < 3; ++axis)
            {
                sortAxis(axis);
                rightArea.assign(t.count + 1, 0.0f);
                float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
                for (uint32_t i = t.count; i-- > 1;)
                {
                    const HostBox& b = boxes[order[t.first + i]];
                    for (int k = 0; k < 3; ++k)
                    {
                        lo[k] = std::min(lo[k], b.lo[k]);
                        hi[k] = std::max(hi[k], b.hi[k]);
                    }
                    rightArea[i] = hb_half_area(lo, hi);
                }
                for (int k = 0; k < 3; ++k)
                {
                    lo[k] = INFINITY;
                    hi[k] = -INFINITY;
                }
                for (uint32_t i = 1; i < t.count; ++i)
                {
                    const HostBox& b = boxes[order[t.first + i - 1]];
                    for (int k = 0; k < 3; ++k)
                    {
                        lo[k] = std::min(lo[k], b.lo[k]);
                        hi[k] = std::max(hi[k], b.hi[k]);
                    }
                    const float cost = hb_half_area(lo, hi) * (float)i + rightArea[i] * (float)(t.count - i);
                    if (cost < bestCost)
                    {
                        bestCost = cost;
                        bestAxis = axis;
                        bestSplit = i;
                    }
                }
            }
            sortAxis(bestAxis);
            ref = (int)bin.size();
            HostBin hbn;
            hbn.left = hbn.right = SKH_REF_INVALID;
            for (int k = 0; k < 3; ++k)
            {
                hbn.lo[k] = INFINITY;
                hbn.hi[k] = -INFINITY;
            }
            for (uint32_t i = t.first; i < t.first + t.count; ++i)
                for (int k = 0; k < 3; ++k)
                {
                    hbn.lo[k] = std::min(hbn.lo[k], boxes[order[i]].lo[k]);
                    hbn.hi[k] = std::max(hbn.hi[k], boxes[order[i]].hi[k]);
                }
            bin.push_back(hbn);
            stack.push_back(Task{ t.first + bestSplit, t.count - bestSplit, ref, 1 });
            stack.push_back(Task{ t.first, bestSplit, ref, 0 });
        }
        if (t.parent < 0)
            rootRef = ref;
        else if (t.side == 0)
            bin[t.parent].left = ref;
        else
            bin[t.parent].right = ref;
    }
    // collapse the binary tree into 4-wide nodes (same greedy rule as k_collapse)
    // (breadth first: node w is work item w, and the children of a level's nodes take the next slots -- levels are contiguous ranges, children behind parents)
    struct Item
    {
        int bin, out, depth;
    };
    std::vector<Item> work;
    nodes.push_back(Node4{});
    work.push_back(Item{ rootRef, 0, 0 });
    for (size_t w = 0; w < work.size(); ++w)
    {
        const Item it = work[w];
        if (levelStart.size() <= (size_t)it.depth)
            levelStart.push_back((uint32_t)w);
        int slot[4];
        int cnt = 2;
        slot[0] = bin[it.bin].left;
        slot[1] = bin[it.bin].right;
        while (cnt < 4)
        {
            int best = -1;
            float bestA = -1.0f;
            for (int k = 0; k < cnt; ++k)
                if (slot[k] >= 0)
                {
                    const float a = hb_half_area(bin[slot[k]].lo, bin[slot[k]].hi);
                    if (a > bestA)
                    {
                        bestA = a;
                        best = k;
                    }
                }
            if (best < 0)
                break;
            const int cidx = slot[best];
            slot[best] = bin[cidx].left;
            slot[cnt++] = bin[cidx].right;
        }
        float clo[4][3], chi[4][3];
        int refs[4];
        for (int k = 0; k < cnt; ++k)
        {
            hb_box_of_ref(slot[k], bin, boxes, clo[k], chi[k]);
            if (slot[k] >= 0)
            {
                refs[k] = (int)nodes.size();
                nodes.push_back(Node4{});
                work.push_back(Item{ slot[k], refs[k], it.depth + 1 });
            }
            else
                refs[k] = slot[k];
        }
        Node4 nd;
        encode_node4(nd, bin[it.bin].lo, bin[it.bin].hi, clo, chi, refs, cnt);
        nodes[it.out] = nd;
    }
    levelStart.push_back((uint32_t)nodes.size());
    return 0; // the root is node 0
}

// the box around the baked light proxies' group from its bounds {lo xyz, hi xyz} (a radiance ray that misses it skips the proxies' tree)
static void set_light_box(skh_context* c, bool any, const float* b6)
{
    // What a visit of the group's root could find must lie inside: encode_node4's margin -- the LARGEST coordinate magnitude over all three axes
    // times 2^-20, the same on every axis (a flat light on the plane x = 0 still gets it: ADVICE r5) -- plus two quantisation cells of the
    // root node per axis (child planes are rounded outward to the node's power-of-two grid, cell < 2 extent / 255).  A larger box only sends
    // a few more rays to the proxies' tree.
    float mAll = 0.0f;
    for (int k = 0; k < 3; ++k)
        mAll = std::max(mAll, std::max(std::fabs(b6[k]), std::fabs(b6[3 + k])));
    for (int k = 0; k < 3; ++k)
    {
        const float ext = (b6[3 + k] + mAll * 0x1p-20f) - (b6[k] - mAll * 0x1p-20f);
        const float m = any ? mAll * 0x1p-20f + 1e-30f + 2.0f * (2.0f * ext / 255.0f) : 0.0f;
        c->accel.lightBox.lo[k] = any ? b6[k] - m : -INFINITY;
        c->accel.lightBox.hi[k] = any ? b6[3 + k] + m : INFINITY;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Launches the build and the in-place update share: both read the tables the last build published in the context.
// ---------------------------------------------------------------------------------------------------------------
// leaf records of the triangle tree, in leaf order (c->accel.nTriSlots of them)
static void launch_gather_tris(skh_context* c)
{
    const uint32_t B = 256;
    k_gather_tris<<<(c->accel.nTriSlots + B - 1) / B, B, 0, c->dev.stream>>>(c->scene.dVerts.as<uint8_t>(), c->scene.dIndices.as<uint32_t>(), c->scene.dMeshes.as<uint4>(), c->accel.dTriMeshK.as<uint32_t>(),
                                                                    c->accel.dTriLocalK.as<uint32_t>(), c->accel.dTriOrder.as<uint32_t>(), c->accel.nTriSlots, c->accel.nMeshTrisBuilt, c->scene.dInstances.as<uint8_t>(),
                                                                    c->accel.dShadeInst.as<uint8_t>(), c->accel.dWInstK.as<uint32_t>(), c->accel.dWFirstK.as<uint32_t>(), c->accel.nWInstBuilt, c->accel.directRecords,
                                                                    c->accel.dTris.as<float4>());
}
// leaf records of the curve tree (control points, bounding cylinders), in leaf order (c->accel.nSubBuilt of them)
static void launch_gather_segs(skh_context* c, uint32_t strandMajor)
{
    const uint32_t B = 256;
    k_gather_segs<<<(c->accel.nSubBuilt + B - 1) / B, B, 0, c->dev.stream>>>(c->scene.dPoints.as<float>(), c->scene.dRadii.as<float>(), c->accel.dSegBuildStartK.as<uint32_t>(), c->accel.dSegLocalK.as<uint32_t>(),
                                                                   c->accel.dSegInstOfK.as<uint32_t>(), c->accel.dSegOrder.as<uint32_t>(), c->accel.nSubBuilt, c->accel.curveSplitBuilt, c->accel.dSegs.as<float4>(), strandMajor);
}
// instance records (c->accel.dDevInst) and world boxes from the BLASes' group roots and bounds (curve set s = group SKH_WORLD_CURVES + s)
static void launch_instance_boxes(skh_context* c, const DevBuf& w2o, const DevBuf& triBounds, const DevBuf& triRoot, const DevBuf& segBounds, const DevBuf& segRoot,
                                  DevBuf& lo, DevBuf& hi, DevBuf& grp)
{
    const uint32_t B = 256, nInst = c->scene.nInstances, nMeshes = (uint32_t)c->scene.meshes.size(), nCurves = (uint32_t)c->scene.curves.size();
    if (!nInst)
        return;
    k_instance_boxes<<<(nInst + B - 1) / B, B, 0, c->dev.stream>>>(c->scene.dInstances.as<HostInstance>(), w2o.as<float>(), c->accel.dBuiltValid.as<uint8_t>(), triBounds.as<float>(),
                                                              triRoot.as<int>(), segBounds.as<float>() + 6 * SKH_WORLD_CURVES, segRoot.as<int>() + SKH_WORLD_CURVES,
                                                              nMeshes, nCurves, nInst, c->accel.dDevInst.as<DevInstance>(), lo.as<float4>(), hi.as<float4>(), grp.as<uint32_t>());
    if (c->opt.tightInstanceBoxes)
        k_instance_tight_boxes<<<nInst, 256, 0, c->dev.stream>>>(c->scene.dInstances.as<HostInstance>(), c->accel.dDevInst.as<DevInstance>(), c->scene.dMeshes.as<uint4>(), c->scene.dVerts.as<uint8_t>(), nMeshes,
                                                             1u << 22, lo.as<float4>(), hi.as<float4>());
}
// boxes of a 4-wide tree level by level, deepest first (skh_bvh.h k_node4_refit_level: one launch per level, no atomics)
template <typename Leaves>
static void launch_refit_levels(skh_context* c, const std::vector<uint32_t>& levelStart, const DevBuf& nodes, const DevBuf& nodeBox, const Leaves& leaves)
{
    const uint32_t B = 256;
    for (size_t L = levelStart.size() > 1 ? levelStart.size() - 1 : 0; L-- > 0;)
    {
        const uint32_t first = levelStart[L], count = levelStart[L + 1] - first;
        if (count)
            k_node4_refit_level<<<(count + B - 1) / B, B, 0, c->dev.stream>>>(nodes.as<Node4>(), nodeBox.as<float4>(), first, count, leaves);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// skh_build_accel: a driver (at the end of this section) over the stages below.  Host stages decide, device stages allocate and launch; what they hand
// each other lives in the driver's scope, so every temporary of the build is freed when the driver returns, on every path.
// ---------------------------------------------------------------------------------------------------------------
static skh_status check_instance_ids(skh_context* c)
{
    for (uint32_t i = 0; i < c->scene.nInstances; ++i)
    {
        // what the kernels index with an instance's ids: a mesh / curve set (traversal, shading) and, for light proxies, a light
        const skh_instance& in = c->scene.instances[i];
        const char* what = nullptr;
        if (in.type > SKH_INSTANCE_CURVE)
            what = "type";
        else if (in.type == SKH_INSTANCE_CURVE ? in.geom_id >= c->scene.curves.size() : in.geom_id >= c->scene.meshes.size())
            what = "geom_id";
        else if (in.type == SKH_INSTANCE_LIGHT && in.light_id >= c->scene.nLights)
            what = "light_id";
        if (what)
        {
            c->dev.err = "skh_build_accel: instance " + std::to_string(i) + " has an out-of-range " + what;
            return SKH_INVALID_ARGUMENT;
        }
    }
    return SKH_OK;
}

// Which instances keep a TLAS leaf, which are baked to world space, which curve instances the world-only kernel walks itself.
// No HIP call in here: an integer rule the CPU checker restates.
struct BakePlan
{
    std::vector<float> w2o;       // 12 per instance (invert_affine)
    std::vector<uint8_t> invOk;   // the transform has a finite inverse
    std::vector<uint8_t> valid;   // ... and the instance takes a TLAS leaf (assign_world_curves clears more; final before it goes to the device)
    std::vector<uint8_t> baked;
    std::vector<uint32_t> meshUsers, meshUsersLeft; // users: mesh + light instances; left: those that keep their TLAS leaf
    // two world-space groups: [0] mesh instances (every ray), [1] light proxies (radiance rays only: shadow rays do not see lights,
    // RAY_MASK_SHADOW, closest_hit.cu:191) -- the ray mask stays a property of the group, not of the triangle
    std::vector<uint32_t> wInst, wFirst;
    uint32_t nBakedG[2] = { 0, 0 };
    bool worldCurves = false;
    std::vector<uint32_t> worldCurveInst; // curve instances with a table entry (and their set's tree) of their own
    std::vector<std::vector<uint32_t>> mergedGroups; // ... and the groups of equal transforms whose segments share one tree each
};
static BakePlan plan_bake(const skh_context* c)
{
    const uint32_t nMeshes = (uint32_t)c->scene.meshes.size(), nInst = c->scene.nInstances;
    BakePlan p;
    std::vector<float>& w2o = p.w2o;
    std::vector<uint8_t>& valid = p.valid;
    std::vector<uint32_t>&meshUsers = p.meshUsers, &meshUsersLeft = p.meshUsersLeft, &wInst = p.wInst, &wFirst = p.wFirst, &worldCurveInst = p.worldCurveInst;
    std::vector<std::vector<uint32_t>>& mergedGroups = p.mergedGroups;
    bool& worldCurves = p.worldCurves;
    uint32_t(&nBakedG)[2] = p.nBakedG;
    w2o.resize(12 * (size_t)std::max(1u, nInst));
    valid.resize(std::max(1u, nInst));
    for (uint32_t i = 0; i < nInst; ++i)
        valid[i] = invert_affine(c->scene.instances[i].transform, &w2o[12 * (size_t)i]) ? 1 : 0;
    p.invOk = valid;
    meshUsers.assign(nMeshes, 0u), meshUsersLeft.assign(nMeshes, 0u);
    p.baked.assign(std::max(1u, nInst), 0);
    uint64_t uniqueTris = 0;
    for (const skh_mesh& me : c->scene.meshes)
        uniqueTris += me.index_count / 3;
    for (uint32_t i = 0; i < nInst; ++i)
        if (c->scene.instances[i].type != SKH_INSTANCE_CURVE && valid[i]) // (a singular instance is disabled: the reference's distant-light proxy is one, of mesh 0, scene.cpp:337-345)
            meshUsers[c->scene.instances[i].geom_id]++;
    const uint64_t smallBudget = std::max<uint64_t>(uniqueTris, 1ull << 20);
    uint64_t total = 0;
    std::vector<uint8_t> pick(std::max(1u, nInst), 0);
    auto trisOf = [&](uint32_t i) { return c->scene.meshes[c->scene.instances[i].geom_id].index_count / 3; };
    auto eligible = [&](uint32_t i) { return c->opt.bakeWorld >= 1 && c->scene.instances[i].type != SKH_INSTANCE_CURVE && valid[i] && trisOf(i) > 0; };
    // mode 4 (default) = everything (3) while the instanced triangles stay within bake_budget_mtris million, else 2: a scene
    // whose instancing fits in memory many times over is fastest with no instancing at all (kitchen stand-in, 23 M instanced
    // triangles = 1.8 GB of leaf records + nodes of 288 GB: closest-hit 98.0 -> 91.0 ms), a forest of 10^9 instanced triangles is not
    uint32_t mode = c->opt.bakeWorld;
    if (mode == 4)
    {
        uint64_t all = 0;
        for (uint32_t i = 0; i < nInst; ++i)
            all += eligible(i) ? trisOf(i) : 0u;
        mode = all <= (uint64_t)c->opt.bakeBudgetMTris * 1000000ull ? 3u : 2u;
    }
    for (uint32_t i = 0; i < nInst; ++i)
        pick[i] = eligible(i) && (meshUsers[c->scene.instances[i].geom_id] == 1 || mode >= 3) ? 1 : 0;
    if (mode == 2)
    {
        // Small SHARED meshes (boards, quads) follow only when that leaves no mesh instance behind: beside a populated top level
        // a partly baked scene measured no faster (kitchen stand-in, any-hit 41.1 -> 42.6 ms), an emptied one saves the level
        bool all = true;
        uint64_t sum = 0;
        for (uint32_t i = 0; i < nInst; ++i)
            if (c->scene.instances[i].type == SKH_INSTANCE_MESH && eligible(i) && !pick[i])
            {
                all = all && trisOf(i) <= c->opt.bakeSmallTris;
                sum += trisOf(i);
            }
        all = all && sum <= smallBudget;
        for (uint32_t i = 0; i < nInst; ++i)
            if (eligible(i) && !pick[i] && trisOf(i) <= c->opt.bakeSmallTris && (all || c->scene.instances[i].type == SKH_INSTANCE_LIGHT))
                pick[i] = 1;
    }
    for (uint32_t i = 0; i < nInst; ++i)
        if (pick[i])
        {
            if (total + trisOf(i) >= (1ull << 27)) // (leaf references address 2^28 primitives)
                pick[i] = 0;
            else
                total += trisOf(i);
        }
    // Light proxies follow the meshes only when that EMPTIES the top level (then no ray ever leaves world space): beside a
    // populated TLAS their own group costs every radiance ray a root visit that the TLAS's distance-ordered culling mostly
    // avoided (kitchen stand-in, closest-hit 99.4 -> 102.4 ms), without a TLAS it saves the whole level (unshared variant: 89.7 -> 81.2 ms)
    // "World curves" (round 5): when a scene holds at most SKH_WORLD_CURVES curve instances with segments (and nothing else needs a top
    // level), their trees are walked straight from the world-only kernel -- no TLAS, no instance-entry pass; the instance's transform is
    // still applied to the ray, by the same operations --, so they do not keep the top level alive either.  An integer rule the CPU
    // checker evaluates too (it decides which light proxies are baked).
    bool meshStays = false;
    std::vector<uint32_t> curveInst;
    for (uint32_t i = 0; i < nInst; ++i)
    {
        const skh_instance& in = c->scene.instances[i];
        if (in.type == SKH_INSTANCE_CURVE)
        {
            uint32_t segs = 0; // (a curve set without a segment has no BLAS and no leaf)
            if (in.geom_id < c->scene.curves.size())
                for (uint32_t k = 0; k < c->scene.curves[in.geom_id].vertex_counts_count; ++k)
                    segs += std::max(3u, c->scene.curveVertexCounts[c->scene.curves[in.geom_id].vertex_counts_start + k]) - 3u;
            if (valid[i] && segs > 0)
                curveInst.push_back(i);
        }
        else if (in.type == SKH_INSTANCE_MESH)
            meshStays = meshStays || (valid[i] && !pick[i] && c->scene.meshes[in.geom_id].index_count >= 3);
    }
    bool lightsAllPicked = true; // (a light proxy the bake mode leaves behind keeps the top level alive as well)
    for (uint32_t i = 0; i < nInst; ++i)
        if (c->scene.instances[i].type == SKH_INSTANCE_LIGHT && eligible(i) && !pick[i])
            lightsAllPicked = false;
    // (round 6) Curve instances under the SAME transform, bit for bit -- a groom handed over as several HdBasisCurves rprims, under the identity or
    // under the one Xform the whole character sits under -- do not take a table entry each: the segments of such a group are MERGED into one
    // curve tree in the group's object space (the first groups of the curve build; the segment records name their instance), which takes ONE
    // entry and is entered through the group's one transform.  Walking 8 / 16 per-prim trees one after the other cost the hair stand-in 33 % /
    // 50 % of its rate (each ray visits every tree's root and whatever overlaps: 40 / 53 instead of 28 nodes per radiance ray), docs/LOG.md.
    std::vector<std::vector<uint32_t>> xformGroups; // curve instances by transform, in order of first appearance
    for (uint32_t i : curveInst)
    {
        size_t g = 0;
        for (; g < xformGroups.size(); ++g)
            if (memcmp(c->scene.instances[xformGroups[g][0]].transform, c->scene.instances[i].transform, sizeof(float) * 12) == 0)
                break;
        if (g == xformGroups.size())
            xformGroups.emplace_back();
        xformGroups[g].push_back(i);
    }
    worldCurves = !meshStays && !curveInst.empty() && xformGroups.size() <= SKH_WORLD_CURVES && lightsAllPicked;
    if (worldCurves)
    {
        // option curve_merge = 0 (A/B, tests): every instance keeps a tree and a table entry of its own while the table can hold them all
        const bool merge = c->opt.curveMerge || curveInst.size() > SKH_WORLD_CURVES;
        if (merge)
            mergedGroups = xformGroups;
        else
            worldCurveInst = curveInst;
    }
    const bool tlasStays = meshStays || (!curveInst.empty() && !worldCurves);
    for (uint32_t i = 0; i < nInst; ++i)
    {
        const skh_instance& in = c->scene.instances[i];
        if (in.type == SKH_INSTANCE_CURVE)
            continue;
        if (in.type == SKH_INSTANCE_LIGHT && tlasStays)
            pick[i] = 0;
        if (!pick[i])
            meshUsersLeft[in.geom_id] += valid[i] ? 1u : 0u;
    }
    total = 0;
    for (uint32_t g = 0; g < 2; ++g)
        for (uint32_t i = 0; i < nInst; ++i)
        {
            const skh_instance& in = c->scene.instances[i];
            if (!pick[i] || (in.type == SKH_INSTANCE_LIGHT ? 1u : 0u) != g)
                continue;
            p.baked[i] = 1;
            valid[i] = 0; // no TLAS leaf
            wInst.push_back(i);
            wFirst.push_back((uint32_t)total);
            const uint32_t nt = c->scene.meshes[in.geom_id].index_count / 3;
            total += nt;
            nBakedG[g] += nt;
        }
    wFirst.push_back((uint32_t)total);
    return p;
}

// the box / group arrays of the triangle build, reused by the curve build and for the instance boxes; the build's world->object table
struct BuildScratch
{
    DevBuf boxLo, boxHi, grp, w2o;
};
struct TriBuild
{
    LbvhOut out;
    DevBuf triMesh, triLocal, wInst, wFirst; // k_gather_tris' tables: swapped into the context for skh_refit_accel (the previous build's die with this one)
    uint32_t nMeshTris = 0, nGroup0 = 0, nGroup1 = 0;
};

// Which word a baked mesh triangle's hit carries.  The index of its shading record (k_shade fetches the record beside the instance's: one short
// step less) -- unless a 16-byte hit record {t, u, v, instance << B | primitive} (compact_hits) has room for the mesh-local index only:
// a closest-hit lane's second scattered store costs more than that step (kitchen closest-hit -4 %).
static void choose_hit_word(skh_context* c)
{
    const uint32_t nMeshes = (uint32_t)c->scene.meshes.size(), nInst = c->scene.nInstances;
    uint32_t maxMeshTris = 1;
    for (uint32_t m = 0; m < nMeshes; ++m)
        maxMeshTris = std::max(maxMeshTris, c->scene.meshes[m].index_count / 3u);
    auto fits = [&](uint32_t range) {
        uint32_t B = 1;
        while (B < 31u && (1u << B) < range)
            ++B;
        return (1ull << B) >= range && (uint64_t)nInst <= (1ull << (32u - B)) - 1ull;
    };
    const uint32_t nSegAll = (uint32_t)std::min<uint64_t>(0x7fffffffull, [&]() { uint64_t n = 0; for (const skh_curve& cu : c->scene.curves) for (uint32_t k = 0; k < cu.vertex_counts_count; ++k) { const uint32_t ncp = c->scene.curveVertexCounts[cu.vertex_counts_start + k]; n += ncp > 3u ? ncp - 3u : 0u; } return n; }());
    const uint32_t rangeDirect = std::max(c->accel.nShadeRecords, nSegAll), rangeLocal = std::max(maxMeshTris, nSegAll);
    c->accel.directRecords = c->opt.directRecords >= 0 ? (uint32_t)c->opt.directRecords : ((c->opt.compactHits && !fits(rangeDirect) && fits(rangeLocal)) ? 0u : 1u);
    c->accel.hitPrimRange = c->accel.directRecords ? rangeDirect : rangeLocal;
}

// triangles of all meshes (a mesh whose users were all baked needs no object-space tree) + the baked groups: boxes, tree, leaf records, roots, light box
static skh_status build_tri_tree(skh_context* c, uint32_t flags, bool usePloc, const BakePlan& p, BuildScratch& sx, TriBuild& tri)
{
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256, nMeshes = (uint32_t)c->scene.meshes.size();
    const uint32_t nBaked = p.nBakedG[0] + p.nBakedG[1], nW = (uint32_t)p.wInst.size();
    std::vector<uint32_t> triMesh, triLocal, meshTriCount(nMeshes + 2u);
    for (uint32_t m = 0; m < nMeshes; ++m)
    {
        const uint32_t nt = (p.meshUsers[m] > 0 && p.meshUsersLeft[m] == 0) ? 0u : c->scene.meshes[m].index_count / 3;
        meshTriCount[m] = nt;
        for (uint32_t t = 0; t < nt; ++t)
        {
            triMesh.push_back(m);
            triLocal.push_back(t);
        }
    }
    // (merge_light_proxies: one world-space group for both kinds -- a light proxy is told from a mesh triangle by its primitive word, which
    // lacks SKH_PRIM_DIRECT (k_gather_tris); any-hit queries, which must not see lights (RAY_MASK_SHADOW, closest_hit.cu:191), skip those triangles)
    const bool mergeLights = c->opt.mergeLightProxies != 0u && p.nBakedG[0] != 0u && p.nBakedG[1] != 0u;
    const uint32_t nGroup0 = mergeLights ? p.nBakedG[0] + p.nBakedG[1] : p.nBakedG[0], nGroup1 = mergeLights ? 0u : p.nBakedG[1];
    meshTriCount[nMeshes] = nGroup0;
    meshTriCount[nMeshes + 1u] = nGroup1;
    const uint32_t nMeshTris = (uint32_t)triMesh.size();
    const uint32_t nTris = nMeshTris + nBaked;
    tri.nMeshTris = nMeshTris, tri.nGroup0 = nGroup0, tri.nGroup1 = nGroup1;
    c->accel.nTris = nTris;
    SKH_CHECK(dev_upload(c, tri.triMesh, triMesh.data(), sizeof(uint32_t) * (size_t)nMeshTris));
    SKH_CHECK(dev_upload(c, tri.triLocal, triLocal.data(), sizeof(uint32_t) * (size_t)nMeshTris));
    SKH_CHECK(dev_upload(c, tri.wInst, p.wInst.data(), sizeof(uint32_t) * p.wInst.size()));
    SKH_CHECK(dev_upload(c, tri.wFirst, p.wFirst.data(), sizeof(uint32_t) * p.wFirst.size()));
    SKH_CHECK(dev_alloc(c, sx.boxLo, sizeof(float4) * (size_t)std::max(1u, nTris)));
    SKH_CHECK(dev_alloc(c, sx.boxHi, sizeof(float4) * (size_t)std::max(1u, nTris)));
    SKH_CHECK(dev_alloc(c, sx.grp, sizeof(uint32_t) * (size_t)std::max(1u, nTris)));
    if (nMeshTris)
        k_tri_boxes<<<(nMeshTris + B - 1) / B, B, 0, st>>>(c->scene.dVerts.as<uint8_t>(), c->scene.dIndices.as<uint32_t>(), c->scene.dMeshes.as<uint4>(),
                                                          tri.triMesh.as<uint32_t>(), tri.triLocal.as<uint32_t>(), nMeshTris, sx.boxLo.as<float4>(),
                                                          sx.boxHi.as<float4>(), sx.grp.as<uint32_t>());
    if (nBaked)
        k_baked_tri_boxes<<<(nBaked + B - 1) / B, B, 0, st>>>(c->scene.dInstances.as<uint8_t>(), tri.wInst.as<uint32_t>(), tri.wFirst.as<uint32_t>(),
                                                             nW, c->scene.dVerts.as<uint8_t>(), c->scene.dIndices.as<uint32_t>(),
                                                             c->scene.dMeshes.as<uint4>(), nBaked, nMeshTris, nMeshes, nGroup0, sx.boxLo.as<float4>(),
                                                             sx.boxHi.as<float4>(), sx.grp.as<uint32_t>());
    const uint32_t riMin = c->opt.reinsertMinSize ? c->opt.reinsertMinSize : (nTris <= (4u << 20) ? 1u : 32u);
    LbvhOut& triOut = tri.out;
    SKH_CHECK(lbvh_build(c, nTris, nMeshes + 2u, meshTriCount, sx.boxLo.as<float4>(), sx.boxHi.as<float4>(), sx.grp.as<uint32_t>(), (int)c->opt.leafMaxTris, usePloc, triOut,
                         0, c->opt.leafLines ? 48u : 0u, usePloc ? c->opt.reinsertRounds : 0u, riMin));
    memset(&c->accel.buildInfo, 0, sizeof(c->accel.buildInfo));
    c->accel.buildInfo.triangles = nTris;
    c->accel.buildInfo.nodes = triOut.numNodes;
    c->accel.hierNodes = triOut.numNodes;
    c->accel.buildInfo.reinsert_rounds = triOut.riRounds;
    c->accel.buildInfo.reinsert_moves = triOut.riMoves;
    c->accel.buildInfo.reinsert_min_size = triOut.riMinSize;
    c->accel.buildInfo.cost_before = triOut.riCostBefore;
    c->accel.buildInfo.cost_after = triOut.riRounds ? triOut.riCostAfter : triOut.riCostBefore;
    c->accel.buildInfo.ms_reinsert = triOut.riMs;
    choose_hit_word(c);
    c->accel.nTriSlots = triOut.numSlots; // >= nTris: the line layout pads in front of leaves that would straddle a 128-byte line
    SKH_CHECK(dev_alloc(c, c->accel.dTris, sizeof(float4) * 3 * (size_t)std::max(1u, c->accel.nTriSlots)));
    // what skh_refit_accel needs of this build: k_gather_tris' tables and the tree's levels (the old ones go out with this call's temporaries)
    std::swap(c->accel.dTriOrder, triOut.sortedVals);
    std::swap(c->accel.dTriMeshK, tri.triMesh);
    std::swap(c->accel.dTriLocalK, tri.triLocal);
    std::swap(c->accel.dWInstK, tri.wInst);
    std::swap(c->accel.dWFirstK, tri.wFirst);
    c->accel.nMeshTrisBuilt = nMeshTris, c->accel.nWInstBuilt = nW;
    if (c->accel.nTriSlots)
        launch_gather_tris(c);
    c->accel.dTriNodes = std::move(triOut.nodes);
    c->accel.triLevelStart = triOut.levelStart;
    c->accel.triNumNodes = triOut.numNodes, c->accel.lastBuildFlags = flags, c->accel.nGroup1Built = nGroup1;
    c->accel.builtGeomSig = c->scene.geomSig, c->accel.builtNVerts = c->scene.nVerts;
    c->accel.refitReady = true; // (either builder ends in the same collapse)
    c->accel.worldRoot = nGroup0 ? triOut.hostGroupRoot[nMeshes] : SKH_REF_INVALID;
    c->accel.lightRoot = nGroup1 ? triOut.hostGroupRoot[nMeshes + 1u] : SKH_REF_INVALID;
    for (int k = 0; k < 3; ++k)
        c->accel.lightBox.lo[k] = -INFINITY, c->accel.lightBox.hi[k] = INFINITY;
    if (nBaked)
    {
        float gb[12];
        SKH_TRY(c, hipMemcpyAsync(gb, triOut.groupBounds.as<float>() + 6 * (size_t)nMeshes, sizeof(gb), hipMemcpyDeviceToHost, st));
        SKH_TRY(c, hipStreamSynchronize(st));
        set_light_box(c, nGroup1 != 0u, gb + 6);
    }
    return SKH_OK;
}

// curve segments of all curve sets (segment enumeration: OptixRender.cpp:226-245), then the curve build's primitives group after group
struct CurveTables
{
    std::vector<uint32_t> setSegStart, curveSegCount, curveSegBase; // per set, set after set: what k_shade looks a hit's control points up in
    std::vector<uint32_t> segStart, segCurve, segLocal, segInstOf, curveGroupCount;
};
static skh_status enumerate_curve_segments(skh_context* c, CurveTables& ct)
{
    const uint32_t nCurves = (uint32_t)c->scene.curves.size();
    std::vector<uint32_t>&setSegStart = ct.setSegStart, &curveSegCount = ct.curveSegCount, &curveSegBase = ct.curveSegBase;
    curveSegCount.resize(nCurves), curveSegBase.resize(nCurves);
    for (uint32_t ci = 0; ci < nCurves; ++ci)
    {
        const skh_curve& cu = c->scene.curves[ci];
        curveSegBase[ci] = (uint32_t)setSegStart.size();
        uint32_t off = 0, local = 0;
        for (uint32_t k = 0; k < cu.vertex_counts_count; ++k)
        {
            const uint32_t ncp = c->scene.curveVertexCounts[cu.vertex_counts_start + k];
            for (int i = 0; i < (int)ncp - 3; ++i, ++local)
                setSegStart.push_back(cu.points_start + off + (uint32_t)i);
            off += ncp;
        }
        curveSegCount[ci] = local;
    }
    for (uint32_t k = 0; k < (uint32_t)setSegStart.size(); ++k)
        if ((uint64_t)setSegStart[k] + 4 > c->scene.nPoints)
        {
            c->dev.err = "skh_build_accel: curve segment reads past the control-point buffer";
            return SKH_INVALID_ARGUMENT;
        }
    return SKH_OK;
}
// The curve build's primitives, group after group: groups [0, SKH_WORLD_CURVES) = the segments of the MERGED transform groups (object space of the
// group's transform; the record names the instance), group SKH_WORLD_CURVES + s = curve set s (skipped when every instance of the set was merged).
static void group_curve_segments(const skh_context* c, const std::vector<std::vector<uint32_t>>& mergedGroups, CurveTables& ct)
{
    const uint32_t nCurves = (uint32_t)c->scene.curves.size(), nInst = c->scene.nInstances;
    const std::vector<uint32_t>&setSegStart = ct.setSegStart, &curveSegCount = ct.curveSegCount, &curveSegBase = ct.curveSegBase;
    std::vector<uint32_t>&segStart = ct.segStart, &segCurve = ct.segCurve, &segLocal = ct.segLocal, &segInstOf = ct.segInstOf, &curveGroupCount = ct.curveGroupCount;
    curveGroupCount.assign(nCurves + SKH_WORLD_CURVES, 0u);
    std::vector<uint8_t> setNeeded(nCurves, mergedGroups.empty() ? 1 : 0);
    if (!mergedGroups.empty())
    {
        std::vector<uint8_t> isMerged(std::max(1u, nInst), 0);
        for (const auto& grp : mergedGroups)
            for (uint32_t i : grp)
                isMerged[i] = 1;
        for (uint32_t i = 0; i < nInst; ++i)
            if (c->scene.instances[i].type == SKH_INSTANCE_CURVE && !isMerged[i] && c->scene.instances[i].geom_id < nCurves)
                setNeeded[c->scene.instances[i].geom_id] = 1;
    }
    for (size_t g = 0; g < mergedGroups.size(); ++g)
        for (uint32_t i : mergedGroups[g])
        {
            const uint32_t ci = c->scene.instances[i].geom_id;
            for (uint32_t l = 0; l < curveSegCount[ci]; ++l)
            {
                segStart.push_back(setSegStart[curveSegBase[ci] + l]);
                segCurve.push_back((uint32_t)g);
                segLocal.push_back(l);
                segInstOf.push_back(i);
            }
            curveGroupCount[g] += curveSegCount[ci];
        }
    for (uint32_t ci = 0; ci < nCurves; ++ci)
        if (setNeeded[ci])
        {
            for (uint32_t l = 0; l < curveSegCount[ci]; ++l)
            {
                segStart.push_back(setSegStart[curveSegBase[ci] + l]);
                segCurve.push_back(SKH_WORLD_CURVES + ci);
                segLocal.push_back(l);
                segInstOf.push_back(0xffffffffu);
            }
            curveGroupCount[SKH_WORLD_CURVES + ci] = curveSegCount[ci];
        }
}

struct CurveBuild
{
    LbvhOut out;
    DevBuf segCurve, segLocal, segBuildStart, segInstOf; // k_gather_segs' tables: swapped into the context for skh_refit_accel
    std::vector<int> setRoot; // root of curve set s's own tree (group SKH_WORLD_CURVES + s)
};

// segment nodes: the tree's nodes, then one segment node per segment; every one-segment leaf reference (internal nodes' child words, the per-set roots) is
// redirected to the segment node in front of the leaf
static skh_status grow_segment_nodes(skh_context* c, uint32_t nSegs, uint32_t nCurveGroups, uint32_t strandMajor, const DevBuf& segBuildStart, LbvhOut& segOut)
{
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256;
    DevBuf grown;
    SKH_CHECK(dev_alloc(c, grown, sizeof(Node4) * ((size_t)segOut.numNodes + nSegs + 1)));
    if (segOut.numNodes)
        SKH_TRY(c, hipMemcpyAsync(grown.p, segOut.nodes.p, sizeof(Node4) * (size_t)segOut.numNodes, hipMemcpyDeviceToDevice, st));
    k_segnode_emit<<<(nSegs + B - 1) / B, B, 0, st>>>(c->scene.dPoints.as<float>(), c->scene.dRadii.as<float>(), segBuildStart.as<uint32_t>(), segOut.sortedVals.as<uint32_t>(), nSegs,
                                                     strandMajor, grown.as<Node4>() + segOut.numNodes);
    if (segOut.numNodes)
        k_segnode_patch<<<(segOut.numNodes * 4u + B - 1) / B, B, 0, st>>>(reinterpret_cast<int*>(grown.p) + 12, segOut.numNodes * 4u, 16u, 4u, segOut.sortedVals.as<uint32_t>(),
                                                                         strandMajor, segOut.numNodes);
    k_segnode_patch<<<(nCurveGroups + B - 1) / B, B, 0, st>>>(segOut.groupRoot.as<int>(), nCurveGroups, 1u, 1u, segOut.sortedVals.as<uint32_t>(), strandMajor, segOut.numNodes);
    SKH_TRY(c, hipMemcpyAsync(segOut.hostGroupRoot.data(), segOut.groupRoot.p, sizeof(int) * (size_t)nCurveGroups, hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    segOut.nodes = std::move(grown);
    segOut.numNodes += nSegs;
    return SKH_OK;
}

static skh_status build_curve_tree(skh_context* c, bool usePloc, const CurveTables& ct, BuildScratch& sx, CurveBuild& cur)
{
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256, nCurves = (uint32_t)c->scene.curves.size();
    const uint32_t nSegs = (uint32_t)ct.segStart.size();
    c->accel.nSegs = nSegs;
    SKH_CHECK(dev_upload(c, c->accel.dSegStartAll, ct.setSegStart.data(), sizeof(uint32_t) * ct.setSegStart.size()));
    SKH_CHECK(dev_upload(c, c->accel.dCurveSegBase, ct.curveSegBase.data(), sizeof(uint32_t) * (size_t)nCurves));
    SKH_CHECK(dev_upload(c, cur.segBuildStart, ct.segStart.data(), sizeof(uint32_t) * (size_t)nSegs));
    SKH_CHECK(dev_upload(c, cur.segInstOf, ct.segInstOf.data(), sizeof(uint32_t) * (size_t)nSegs));
    SKH_CHECK(dev_upload(c, cur.segCurve, ct.segCurve.data(), sizeof(uint32_t) * (size_t)nSegs));
    SKH_CHECK(dev_upload(c, cur.segLocal, ct.segLocal.data(), sizeof(uint32_t) * (size_t)nSegs));
    const bool segNode = c->opt.curveSegNode != 0 && nSegs > 0;
    const uint32_t K = segNode ? 1u : std::max(1u, std::min(c->opt.curveSplit, 8u)); // (segment nodes: the tree's primitives are whole segments)
    if ((uint64_t)nSegs * K >= (1ull << 28) || (segNode && (uint64_t)nSegs * 2 >= (1ull << 28)))
    {
        c->dev.err = "skh_build_accel: more than 2^28 curve sub-segments (lower the curve_split option)";
        return SKH_INVALID_ARGUMENT;
    }
    const uint32_t nSub = nSegs * K;
    const uint32_t nCurveGroups = nCurves + SKH_WORLD_CURVES; // [0, SKH_WORLD_CURVES) the merged transform groups, [SKH_WORLD_CURVES + s] curve set s
    std::vector<uint32_t> curveSubCount(nCurveGroups);
    for (uint32_t g = 0; g < nCurveGroups; ++g)
        curveSubCount[g] = ct.curveGroupCount[g] * K;
    SKH_CHECK(dev_alloc(c, sx.boxLo, sizeof(float4) * (size_t)std::max(nSub, std::max(1u, c->scene.nInstances))));
    SKH_CHECK(dev_alloc(c, sx.boxHi, sizeof(float4) * (size_t)std::max(nSub, std::max(1u, c->scene.nInstances))));
    SKH_CHECK(dev_alloc(c, sx.grp, sizeof(uint32_t) * (size_t)std::max(nSub, std::max(1u, c->scene.nInstances))));
    if (nSub && segNode)
        k_seg_union_boxes<<<(nSegs + B - 1) / B, B, 0, st>>>(c->scene.dPoints.as<float>(), c->scene.dRadii.as<float>(), cur.segBuildStart.as<uint32_t>(),
                                                            cur.segCurve.as<uint32_t>(), nSegs, sx.boxLo.as<float4>(), sx.boxHi.as<float4>(), sx.grp.as<uint32_t>());
    else if (nSub)
        k_seg_boxes<<<(nSub + B - 1) / B, B, 0, st>>>(c->scene.dPoints.as<float>(), c->scene.dRadii.as<float>(), cur.segBuildStart.as<uint32_t>(),
                                                      cur.segCurve.as<uint32_t>(), nSub, K, sx.boxLo.as<float4>(), sx.boxHi.as<float4>(),
                                                      sx.grp.as<uint32_t>());
    LbvhOut& segOut = cur.out;
    SKH_CHECK(lbvh_build(c, nSub, nCurveGroups, curveSubCount, sx.boxLo.as<float4>(), sx.boxHi.as<float4>(), sx.grp.as<uint32_t>(), segNode ? 1 : (int)c->opt.curveLeaf, usePloc, segOut, 2, 0u,
                         usePloc ? c->opt.reinsertCurveRounds : 0u, c->opt.reinsertMinSize ? c->opt.reinsertMinSize : (nSub <= (8u << 20) ? 1u : 32u)));
    const uint32_t strandMajor = segNode && c->opt.curveStrandMajor ? 1u : 0u;
    if (segNode)
        SKH_CHECK(grow_segment_nodes(c, nSegs, nCurveGroups, strandMajor, cur.segBuildStart, segOut));
    SKH_CHECK(dev_alloc(c, c->accel.dSegs, sizeof(float4) * SKH_SEG_STRIDE * (size_t)std::max(1u, nSub)));
    // what skh_refit_accel needs of the curve build (segment nodes carry boxes of their own kind: no refit for that experimental build)
    std::swap(c->accel.dSegOrder, segOut.sortedVals);
    std::swap(c->accel.dSegBuildStartK, cur.segBuildStart);
    std::swap(c->accel.dSegLocalK, cur.segLocal);
    std::swap(c->accel.dSegInstOfK, cur.segInstOf);
    c->accel.nSubBuilt = nSub, c->accel.curveSplitBuilt = K;
    if (nSub)
        launch_gather_segs(c, strandMajor);
    c->accel.dSegNodes = std::move(segOut.nodes);
    c->accel.hierNodes += segOut.numNodes;
    c->accel.segLevelStart = segOut.levelStart;
    c->accel.segNumNodes = segOut.numNodes;
    c->accel.builtCurveSig = c->scene.curveSig, c->accel.curvePointsEdited = false;
    c->accel.curveRefitReady = !segNode;
    cur.setRoot.assign(nCurves, SKH_REF_INVALID);
    for (uint32_t ci = 0; ci < nCurves; ++ci)
        cur.setRoot[ci] = segOut.hostGroupRoot[SKH_WORLD_CURVES + ci];
    return SKH_OK;
}

// world curves: walked from the world-only kernel (option world_kernel; without it they keep their TLAS leaves: same hit records).  Runs BEFORE the
// validity flags go to the device: both TLAS builders then agree on which instances have a leaf (ADVICE r5).
static void assign_world_curves(skh_context* c, bool worldCurveKernel, BakePlan& p, const CurveBuild& cur)
{
    const uint32_t nCurves = (uint32_t)c->scene.curves.size();
    const std::vector<int>&curveSetRoot = cur.setRoot, &mergedRoot = cur.out.hostGroupRoot;
    std::vector<uint32_t>& worldCurveInst = p.worldCurveInst;
    const std::vector<std::vector<uint32_t>>& mergedGroups = p.mergedGroups;
    std::vector<uint8_t>& valid = p.valid;
    c->accel.numWorldCurves = 0;
    c->accel.worldCurveIdentLast = 0;
    c->accel.worldCurveMerged = 0;
    c->accel.numMergedCurveInst = 0;
    if (worldCurveKernel)
    {
        // (an entry under a bit-exact identity transform goes LAST in the table = first off every ray's stack: the kernel skips its matrix fetch)
        static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        for (size_t k = 0; k + 1 < worldCurveInst.size(); ++k)
            if (memcmp(c->scene.instances[worldCurveInst[k]].transform, kIdentity, sizeof(kIdentity)) == 0)
            {
                std::swap(worldCurveInst[k], worldCurveInst.back());
                break;
            }
        for (uint32_t i : worldCurveInst)
        {
            const int root = c->scene.instances[i].geom_id < nCurves ? curveSetRoot[c->scene.instances[i].geom_id] : SKH_REF_INVALID;
            if (root == SKH_REF_INVALID)
                continue;
            c->accel.worldCurveRoot[c->accel.numWorldCurves] = root;
            c->accel.worldCurveInst[c->accel.numWorldCurves++] = i;
            c->accel.worldCurveIdentLast = memcmp(c->scene.instances[i].transform, kIdentity, sizeof(kIdentity)) == 0 ? 1u : 0u; // (of the last one entered)
            valid[i] = 0; // no TLAS leaf
        }
        std::vector<size_t> order; // merged groups: the identity group last
        for (size_t g = 0; g < mergedGroups.size(); ++g)
            if (memcmp(c->scene.instances[mergedGroups[g][0]].transform, kIdentity, sizeof(kIdentity)) != 0)
                order.push_back(g);
        for (size_t g = 0; g < mergedGroups.size(); ++g)
            if (memcmp(c->scene.instances[mergedGroups[g][0]].transform, kIdentity, sizeof(kIdentity)) == 0)
                order.push_back(g);
        for (size_t g : order)
        {
            for (uint32_t i : mergedGroups[g])
                valid[i] = 0;
            if (mergedRoot[g] == SKH_REF_INVALID)
                continue;
            c->accel.worldCurveMerged |= 1u << c->accel.numWorldCurves; // = "the segment record names the instance" (DevScene::segInst); the entry's instance lends its transform
            c->accel.worldCurveRoot[c->accel.numWorldCurves] = mergedRoot[g];
            c->accel.worldCurveInst[c->accel.numWorldCurves++] = mergedGroups[g][0];
            c->accel.worldCurveIdentLast = memcmp(c->scene.instances[mergedGroups[g][0]].transform, kIdentity, sizeof(kIdentity)) == 0 ? 1u : 0u;
            c->accel.numMergedCurveInst += (uint32_t)mergedGroups[g].size();
        }
    }
}

// instance records and boxes (baked instances and world curves were marked invalid above: they get a record for shading, no leaf)
static skh_status build_instance_boxes(skh_context* c, const BakePlan& p, const TriBuild& tri, const CurveBuild& cur, BuildScratch& sx)
{
    SKH_CHECK(dev_upload(c, sx.w2o, p.w2o.data(), sizeof(float) * p.w2o.size()));
    SKH_CHECK(dev_upload(c, c->accel.dBuiltValid, p.valid.data(), p.valid.size()));
    SKH_CHECK(dev_alloc(c, c->accel.dDevInst, sizeof(DevInstance) * (size_t)std::max(1u, c->scene.nInstances)));
    launch_instance_boxes(c, sx.w2o, tri.out.groupBounds, tri.out.groupRoot, cur.out.groupBounds, cur.out.groupRoot, sx.boxLo, sx.boxHi, sx.grp);
    return SKH_OK;
}

// TLAS on the GPU: the same PLOC + 4-wide collapse that builds the BLASes, over the instance boxes.  Which instances
// take part is known on the host without reading anything back: a finite inverse and a non-empty BLAS.
static skh_status build_tlas_gpu(skh_context* c, const BakePlan& p, const TriBuild& tri, const CurveBuild& cur, const BuildScratch& sx)
{
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256, nInst = c->scene.nInstances;
    std::vector<uint32_t> leafInst;
    for (uint32_t i = 0; i < nInst; ++i)
    {
        const skh_instance& in = c->scene.instances[i];
        const std::vector<int>& roots = in.type == SKH_INSTANCE_CURVE ? cur.setRoot : tri.out.hostGroupRoot;
        if (p.valid[i] && in.geom_id < roots.size() && roots[in.geom_id] != SKH_REF_INVALID)
            leafInst.push_back(i);
    }
    const uint32_t nLeaves = (uint32_t)leafInst.size();
    c->accel.numTlasLeaves = nLeaves;
    dev_free(c->accel.dTlasNodes);
    dev_free(c->accel.dTlasInst);
    c->accel.tlasLevelStart.clear();
    if (nLeaves == 0)
    {
        dev_free(c->accel.dTravInst);
        c->accel.tlasRoot = SKH_REF_INVALID;
        return SKH_OK;
    }
    DevBuf dLeafInst, dLeafLo, dLeafHi, dLeafGrp, dTinstTmp;
    LbvhOut tlasOut;
    SKH_CHECK(dev_upload(c, dLeafInst, leafInst.data(), sizeof(uint32_t) * (size_t)nLeaves));
    SKH_CHECK(dev_alloc(c, dLeafLo, sizeof(float4) * (size_t)nLeaves));
    SKH_CHECK(dev_alloc(c, dLeafHi, sizeof(float4) * (size_t)nLeaves));
    SKH_CHECK(dev_alloc(c, dLeafGrp, sizeof(uint32_t) * (size_t)nLeaves));
    SKH_CHECK(dev_alloc(c, dTinstTmp, sizeof(DevInstance) * (size_t)nLeaves));
    SKH_CHECK(dev_alloc(c, c->accel.dTravInst, sizeof(DevInstance) * (size_t)nLeaves));
    k_tlas_leaves<<<(nLeaves + B - 1) / B, B, 0, st>>>(dLeafInst.as<uint32_t>(), nLeaves, c->accel.dDevInst.as<DevInstance>(), sx.boxLo.as<float4>(),
                                                       sx.boxHi.as<float4>(), dLeafLo.as<float4>(), dLeafHi.as<float4>(), dLeafGrp.as<uint32_t>(),
                                                       dTinstTmp.as<DevInstance>());
    SKH_CHECK(lbvh_build(c, nLeaves, 1, std::vector<uint32_t>{ nLeaves }, dLeafLo.as<float4>(), dLeafHi.as<float4>(), dLeafGrp.as<uint32_t>(), 1, true, tlasOut, 1));
    // traversal records into leaf order (a TLAS leaf ref carries its position: sc.tinst + first)
    k_permute_instances<<<(nLeaves + B - 1) / B, B, 0, st>>>(dTinstTmp.as<DevInstance>(), tlasOut.sortedVals.as<uint32_t>(), nLeaves,
                                                             c->accel.dTravInst.as<DevInstance>());
    c->accel.tlasRoot = tlasOut.hostGroupRoot[0];
    c->accel.dTlasNodes = std::move(tlasOut.nodes);
    c->accel.tlasLevelStart = tlasOut.levelStart; // (skh_update_accel refits the TLAS level by level; its leaf order is the one dTravInst holds)
    if (getenv("SKH_DEBUG"))
        fprintf(stderr, "[skh] TLAS (GPU PLOC): %u instances, %u leaves, %u nodes, root %d\n", nInst, nLeaves, tlasOut.numNodes, c->accel.tlasRoot);
    return SKH_OK;
}

// ---- TLAS opening (partial re-braiding) ----
// A TLAS leaf is (instance, BLAS subtree).  Starting from one leaf per instance, the leaf with the largest world
// box is replaced by the children of its subtree's root until the budget is used: big instances that contain or
// overlap others (rooms, floors, rotated boxes) stop dragging every ray through their whole box.  Results do not
// depend on it (closest hit = min t, ties by (instance, primitive)); only nodes / instance entries per ray do.
// Output: the leaves' boxes, their ids (0, 1, ...) and traversal records (one per TLAS leaf; pad = id of the instance it belongs to).
static skh_status open_tlas_leaves(skh_context* c, const std::vector<DevInstance>& hinst, const std::vector<float4>& hlo, const std::vector<float4>& hhi,
                                   std::vector<HostBox>& hb, std::vector<uint32_t>& ids, std::vector<DevInstance>& tinst)
{
    const uint32_t nInst = c->scene.nInstances;
    std::vector<Node4> hTri, hSeg;
    const bool open = c->opt.tlasOpen > 1;
    if (open)
    {
        hTri.resize(c->accel.triNumNodes);
        hSeg.resize(c->accel.segNumNodes);
        if (!hTri.empty())
            SKH_TRY(c, hipMemcpy(hTri.data(), c->accel.dTriNodes.p, sizeof(Node4) * hTri.size(), hipMemcpyDeviceToHost));
        if (!hSeg.empty())
            SKH_TRY(c, hipMemcpy(hSeg.data(), c->accel.dSegNodes.p, sizeof(Node4) * hSeg.size(), hipMemcpyDeviceToHost));
    }
    struct Ref
    {
        uint32_t inst;
        int node;
        HostBox box;
        float area;
    };
    auto areaOf = [](const HostBox& b) { return hb_half_area(b.lo, b.hi); };
    auto cmp = [](const Ref& a, const Ref& b) { return a.area < b.area || (a.area == b.area && a.inst > b.inst); };
    std::vector<Ref> heap, done;
    uint32_t nValid = 0;
    for (uint32_t i = 0; i < nInst; ++i)
        if (hinst[i].mask != 0)
        {
            Ref r{ i, hinst[i].rootRef, HostBox{ { hlo[i].x, hlo[i].y, hlo[i].z }, { hhi[i].x, hhi[i].y, hhi[i].z } }, 0.0f };
            r.area = areaOf(r.box);
            heap.push_back(r);
            ++nValid;
        }
    std::make_heap(heap.begin(), heap.end(), cmp);
    const size_t budget = open ? (size_t)nValid * c->opt.tlasOpen : (size_t)nValid;
    while (!heap.empty())
    {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        const Ref r = heap.back();
        heap.pop_back();
        const std::vector<Node4>& bn = hinst[r.inst].type == 2 ? hSeg : hTri;
        if (!open || r.node < 0 || r.node == SKH_REF_INVALID || (size_t)r.node >= bn.size() || heap.size() + done.size() + 4 > budget)
        {
            done.push_back(r);
            continue;
        }
        const Node4& nd = bn[(size_t)r.node];
        const float* M = c->scene.instances[r.inst].transform; // object -> world, 3x4 row-major
        for (int ch = 0; ch < 4; ++ch)
        {
            if (nd.child[ch] == SKH_REF_INVALID)
                continue;
            // child box in object space (decoded as the traversal kernel sees it), padded, then the box of its
            // eight transformed corners, padded again and clipped to the parent leaf's box
            double lo[3], hi[3];
            for (int a = 0; a < 3; ++a)
            {
                const double cell = (double)(a == 0 ? nd.cellx : (a == 1 ? nd.celly : nd.cellz));
                lo[a] = (double)nd.o[a] + cell * (double)((nd.qlo[a] >> (8 * ch)) & 0xffu);
                hi[a] = (double)nd.o[a] + cell * (double)((nd.qhi[a] >> (8 * ch)) & 0xffu);
                const double pad = (std::fabs(lo[a]) + std::fabs(hi[a])) * 0x1p-20 + 1e-30;
                lo[a] -= pad;
                hi[a] += pad;
            }
            Ref q{ r.inst, nd.child[ch], HostBox{ { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY } }, 0.0f };
            for (int k = 0; k < 8; ++k)
            {
                const double x = (k & 1) ? hi[0] : lo[0], y = (k & 2) ? hi[1] : lo[1], z = (k & 4) ? hi[2] : lo[2];
                for (int a = 0; a < 3; ++a)
                {
                    const double w = (double)M[4 * a] * x + (double)M[4 * a + 1] * y + (double)M[4 * a + 2] * z + (double)M[4 * a + 3];
                    const double pad = std::fabs(w) * 0x1p-20 + 1e-30;
                    q.box.lo[a] = std::min(q.box.lo[a], (float)(w - pad));
                    q.box.hi[a] = std::max(q.box.hi[a], (float)(w + pad));
                }
            }
            for (int a = 0; a < 3; ++a)
            {
                q.box.lo[a] = std::max(q.box.lo[a], r.box.lo[a]);
                q.box.hi[a] = std::min(q.box.hi[a], r.box.hi[a]);
                if (q.box.hi[a] < q.box.lo[a])
                    q.box.hi[a] = q.box.lo[a];
            }
            q.area = areaOf(q.box);
            heap.push_back(q);
            std::push_heap(heap.begin(), heap.end(), cmp);
        }
    }
    // deterministic leaf numbering: by (instance, node)
    std::sort(done.begin(), done.end(), [](const Ref& a, const Ref& b) { return a.inst < b.inst || (a.inst == b.inst && a.node < b.node); });
    hb.resize(done.size());
    tinst.resize(std::max<size_t>(1, done.size()));
    for (size_t r = 0; r < done.size(); ++r)
    {
        hb[r] = done[r].box;
        ids.push_back((uint32_t)r);
        tinst[r] = hinst[done[r].inst];
        tinst[r].rootRef = done[r].node;
        tinst[r].pad = done[r].inst;
    }
    c->accel.numTlasLeaves = (uint32_t)done.size();
    return SKH_OK;
}

// TLAS on the host: the instance boxes were produced on the device (k_instance_boxes); the sweep runs on the host
static skh_status build_tlas_host(skh_context* c, const BuildScratch& sx)
{
    const uint32_t nInst = c->scene.nInstances;
    std::vector<float4> hlo(nInst), hhi(nInst);
    std::vector<DevInstance> hinst(nInst);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(hlo.data(), sx.boxLo.p, sizeof(float4) * nInst, hipMemcpyDeviceToHost));
    SKH_TRY(c, hipMemcpy(hhi.data(), sx.boxHi.p, sizeof(float4) * nInst, hipMemcpyDeviceToHost));
    SKH_TRY(c, hipMemcpy(hinst.data(), c->accel.dDevInst.p, sizeof(DevInstance) * nInst, hipMemcpyDeviceToHost));
    std::vector<HostBox> hb;
    std::vector<uint32_t> ids;
    std::vector<DevInstance> tinst;
    SKH_CHECK(open_tlas_leaves(c, hinst, hlo, hhi, hb, ids, tinst));
    SKH_CHECK(dev_upload(c, c->accel.dTravInst, tinst.data(), sizeof(DevInstance) * tinst.size()));
    std::vector<Node4> hnodes;
    std::vector<uint32_t> horder;
    c->accel.tlasRoot = tlas_sah_build(hb, ids, hnodes, horder, c->accel.tlasLevelStart);
    if (getenv("SKH_DEBUG"))
    {
        fprintf(stderr, "[skh] TLAS: %u instances, %zu leaves, %zu nodes, root %d\n", nInst, ids.size(), hnodes.size(), c->accel.tlasRoot);
        for (uint32_t i = 0; i < std::min((uint32_t)hb.size(), 8u); ++i)
            fprintf(stderr, "[skh]  leaf %u inst %u root %d box %g %g %g .. %g %g %g\n", i, tinst[i].pad, tinst[i].rootRef, hb[i].lo[0], hb[i].lo[1], hb[i].lo[2], hb[i].hi[0], hb[i].hi[1], hb[i].hi[2]);
    }
    dev_free(c->accel.dTlasNodes);
    dev_free(c->accel.dTlasInst);
    SKH_CHECK(dev_upload(c, c->accel.dTlasNodes, hnodes.data(), sizeof(Node4) * hnodes.size()));
    SKH_CHECK(dev_upload(c, c->accel.dTlasInst, horder.data(), sizeof(uint32_t) * horder.size()));
    return SKH_OK;
}

skh_status skh_build_accel(skh_context* c, uint32_t flags)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(build_shading_tables(c));
    SKH_CHECK(check_instance_ids(c));
    c->accel.updateReady = false;
    const bool usePloc = (flags & SKH_BUILD_SAH) != 0 || c->opt.buildQuality != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t nInst = c->scene.nInstances;
    BakePlan plan = plan_bake(c);
    c->accel.builtInvOk = plan.invOk;
    c->accel.baked = plan.baked;
    c->accel.nBakedTris = plan.nBakedG[0] + plan.nBakedG[1];
    c->accel.nBakedInst = (uint32_t)plan.wInst.size();
    // (declared before the stages run: whatever a stage allocated is freed when this function returns, by any exit)
    BuildScratch sx;
    TriBuild tri;
    CurveBuild cur;
    CurveTables ct;
    SKH_CHECK(build_tri_tree(c, flags, usePloc, plan, sx, tri));
    SKH_CHECK(enumerate_curve_segments(c, ct));
    // Is anything else going to keep a top-level leaf?  (By the bake plan's rule nothing does when worldCurves holds; checked, not assumed: a curve instance
    // without a leaf AND without the world-only kernel would vanish.)  Decided HERE, before the curve build and before the validity flags go to the device
    // (the host-sweep TLAS path picks its leaves by the device's flags: ADVICE r5).
    bool othersInTlas = false;
    for (uint32_t i = 0; i < nInst; ++i)
        if (plan.valid[i] && c->scene.instances[i].type != SKH_INSTANCE_CURVE)
        {
            const std::vector<int>& roots = tri.out.hostGroupRoot;
            othersInTlas = othersInTlas || (c->scene.instances[i].geom_id < roots.size() && roots[c->scene.instances[i].geom_id] != SKH_REF_INVALID);
        }
    const bool worldCurveKernel = plan.worldCurves && c->opt.worldKernel && !othersInTlas;
    if (!worldCurveKernel)
        plan.mergedGroups.clear(); // (every curve instance keeps its TLAS leaf and its set's own tree)
    c->accel.builtMergedGroups = plan.mergedGroups;
    group_curve_segments(c, plan.mergedGroups, ct);
    SKH_CHECK(build_curve_tree(c, usePloc, ct, sx, cur));
    assign_world_curves(c, worldCurveKernel, plan, cur); // (plan.valid is final from here on)
    SKH_CHECK(build_instance_boxes(c, plan, tri, cur, sx));
    uint32_t nValidHost = 0;
    for (uint32_t i = 0; i < nInst; ++i)
        nValidHost += plan.valid[i] ? 1u : 0u;
    const bool tlasOnGpu = c->opt.tlasBuild == 1 || (c->opt.tlasBuild == 2 && nValidHost > 8192u);
    if (nInst > 0 && tlasOnGpu && c->opt.tlasOpen <= 1)
        SKH_CHECK(build_tlas_gpu(c, plan, tri, cur, sx));
    else if (nInst > 0)
        SKH_CHECK(build_tlas_host(c, sx));
    else
    {
        dev_free(c->accel.dTlasNodes);
        dev_free(c->accel.dTlasInst);
        dev_free(c->accel.dTravInst);
        c->accel.tlasRoot = SKH_REF_INVALID;
        c->accel.tlasLevelStart.clear();
    }
    if (getenv("SKH_DEBUG"))
        fprintf(stderr, "[skh] bake_world %u: %u of %u instances baked, %u + %u world-space triangles, roots %d %d; %u object-space triangles; TLAS root %d\n", c->opt.bakeWorld,
                c->accel.nBakedInst, nInst, plan.nBakedG[0], plan.nBakedG[1], c->accel.worldRoot, c->accel.lightRoot, tri.nMeshTris, c->accel.tlasRoot);
    // k_instance_boxes' inputs for skh_update_accel (the previous build's are freed with this call's temporaries)
    std::swap(c->accel.dTriGroupRoot, tri.out.groupRoot);
    std::swap(c->accel.dTriGroupBounds, tri.out.groupBounds);
    std::swap(c->accel.dSegGroupRoot, cur.out.groupRoot);
    std::swap(c->accel.dSegGroupBounds, cur.out.groupBounds);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipGetLastError());
    c->accel.built = true;
    c->accel.builtInstances = c->scene.instances;
    c->accel.vertsEdited = false;
    c->accel.updateReady = true;
    c->accel.msBuild = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SKH_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// In-place updates: skh_refit_accel (round 6: a VERTEX edit of a scene without a top level) and skh_update_accel (instance TRANSFORMS, vertices and curve
// control points, in any combination, for every scene kind) share ONE routine.  Every hierarchy keeps its topology; the build's own pieces recompute the rest:
//   - the triangle tree (object-space BLASes + the baked world-space groups, which carry the instance transforms): leaf records gathered again by k_gather_tris,
//     boxes level by level, deepest first (skh_bvh.h k_node4_refit_level: one launch per level, no atomics); the curve tree likewise;
//   - the BLASes' root boxes (k_ref_boxes over the group roots) replace the build's group bounds;
//   - the instance records (w2o by invert_affine, the build's bits) and world boxes: k_instance_boxes (+ k_instance_tight_boxes);
//   - the TLAS: its traversal records rewritten (k_tlas_records), its boxes refitted level by level from the new instance boxes (TlasLeaves);
//   - the light box; the shading tables.
// Hit records do not depend on the hierarchy: the updated trees return what a rebuild returns, only the nodes visited per ray differ
// (tests/test_gpu_parity.py::test_refit_after_a_vertex_edit_equals_a_rebuild, tests/test_gpu_update.py).
// ---------------------------------------------------------------------------------------------------------------
static skh_status update_stages(skh_context* c, bool verts, bool moved, const std::vector<float>& w2o, uint32_t kind)
{
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = c->dev.stream;
    const uint32_t B = 256;
    const uint32_t nInst = c->scene.nInstances, nMeshes = (uint32_t)c->scene.meshes.size(), nCurves = (uint32_t)c->scene.curves.size();
    DevBuf dRefs, dOut;
    if (nInst != c->accel.builtInstances.size() || c->scene.instances.size() != nInst)
    {
        // (the records below -- dDevInst, the validity flags, the TLAS leaves -- are the build's, sized by its instance count; the callers admit nothing else)
        c->dev.err = std::string(kind == 1 ? "skh_refit_accel" : "skh_update_accel") + ": the instance table does not have the built count";
        return SKH_INVALID_ARGUMENT;
    }
    SKH_CHECK(build_shading_tables(c)); // (normals, tangents, uvs may have changed with the positions; the instance copy carries the transforms)
    // ---- bottom level: the triangle tree (baked world-space triangles move with their instances) and the curve tree ----
    const bool tris = (verts || (moved && c->accel.nBakedTris > 0)) && c->accel.nTriSlots > 0;
    if (tris)
    {
        launch_gather_tris(c);
        SKH_CHECK(dev_alloc(c, c->accel.dTriNodeBox, sizeof(float4) * 2 * (size_t)std::max(1u, c->accel.triNumNodes)));
        const TriLeaves leaves{ c->accel.dTris.as<float4>() };
        launch_refit_levels(c, c->accel.triLevelStart, c->accel.dTriNodes, c->accel.dTriNodeBox, leaves);
        // the BLASes' root boxes: k_instance_boxes' input from now on
        k_ref_boxes<<<(nMeshes + 2u + 63u) / 64u, 64, 0, st>>>(c->accel.dTriGroupRoot.as<int>(), nMeshes + 2u, leaves, c->accel.dTriNodeBox.as<float4>(), c->accel.dTriGroupBounds.as<float>());
    }
    const bool segs = c->accel.curvePointsEdited && c->accel.nSubBuilt > 0;
    if (segs)
    {
        // leaf records (control points, bounding cylinders) gathered again from the new points, boxes level by level
        launch_gather_segs(c, 0u);
        SKH_CHECK(dev_alloc(c, c->accel.dSegNodeBox, sizeof(float4) * 2 * (size_t)std::max(1u, c->accel.segNumNodes)));
        const CurveLeaves leaves{ c->accel.dSegs.as<float4>(), c->accel.curveSplitBuilt };
        launch_refit_levels(c, c->accel.segLevelStart, c->accel.dSegNodes, c->accel.dSegNodeBox, leaves);
        k_ref_boxes<<<(nCurves + SKH_WORLD_CURVES + 63u) / 64u, 64, 0, st>>>(c->accel.dSegGroupRoot.as<int>(), nCurves + SKH_WORLD_CURVES, leaves, c->accel.dSegNodeBox.as<float4>(),
                                                                             c->accel.dSegGroupBounds.as<float>());
    }
    c->accel.curvePointsEdited = false;
    // ---- instance records and boxes, then the top level ----
    const bool tlas = c->accel.tlasRoot != SKH_REF_INVALID && nInst > 0 && (moved || tris || segs); // (the instance stage runs, and with it the TLAS refit)
    if (nInst > 0 && (moved || tlas))
    {
        std::vector<float> w2oNow;
        const std::vector<float>* W = &w2o;
        if (w2o.size() < 12 * (size_t)nInst)
        {
            w2oNow.resize(12 * (size_t)nInst);
            for (uint32_t i = 0; i < nInst; ++i)
                (void)invert_affine(c->scene.instances[i].transform, &w2oNow[12 * (size_t)i]);
            W = &w2oNow;
        }
        SKH_CHECK(dev_upload(c, c->accel.dW2o, W->data(), sizeof(float) * 12 * (size_t)nInst));
        SKH_CHECK(dev_alloc(c, c->accel.dInstLo, sizeof(float4) * (size_t)nInst));
        SKH_CHECK(dev_alloc(c, c->accel.dInstHi, sizeof(float4) * (size_t)nInst));
        SKH_CHECK(dev_alloc(c, c->accel.dInstGrp, sizeof(uint32_t) * (size_t)nInst));
        launch_instance_boxes(c, c->accel.dW2o, c->accel.dTriGroupBounds, c->accel.dTriGroupRoot, c->accel.dSegGroupBounds, c->accel.dSegGroupRoot, c->accel.dInstLo, c->accel.dInstHi, c->accel.dInstGrp);
        if (tlas)
        {
            k_tlas_records<<<(c->accel.numTlasLeaves + B - 1) / B, B, 0, st>>>(c->accel.dTravInst.as<DevInstance>(), c->accel.numTlasLeaves, c->accel.dDevInst.as<DevInstance>());
            const uint32_t nNodes = c->accel.tlasLevelStart.empty() ? 0u : c->accel.tlasLevelStart.back();
            SKH_CHECK(dev_alloc(c, c->accel.dTlasNodeBox, sizeof(float4) * 2 * (size_t)std::max(1u, nNodes)));
            const TlasLeaves leaves{ c->accel.dTravInst.as<DevInstance>(), c->accel.dInstLo.as<float4>(), c->accel.dInstHi.as<float4>() };
            launch_refit_levels(c, c->accel.tlasLevelStart, c->accel.dTlasNodes, c->accel.dTlasNodeBox, leaves);
        }
    }
    // ---- the box the host keeps: around the baked light proxies (radiance rays that miss it skip their tree) ----
    float gb[12];
    if (tris)
    {
        const int refs[2] = { c->accel.worldRoot, c->accel.lightRoot };
        SKH_CHECK(dev_upload(c, dRefs, refs, sizeof(refs)));
        SKH_CHECK(dev_alloc(c, dOut, sizeof(gb)));
        k_ref_boxes<<<1, 64, 0, st>>>(dRefs.as<int>(), 2u, TriLeaves{ c->accel.dTris.as<float4>() }, c->accel.dTriNodeBox.as<float4>(), dOut.as<float>()); // (INVALID roots give empty boxes)
        SKH_TRY(c, hipMemcpyAsync(gb, dOut.p, sizeof(gb), hipMemcpyDeviceToHost, st));
    }
    SKH_TRY(c, hipStreamSynchronize(st));
    SKH_TRY(c, hipGetLastError());
    if (tris)
        set_light_box(c, c->accel.lightRoot != SKH_REF_INVALID && c->accel.nGroup1Built != 0u, gb + 6);
    c->accel.builtInstances = c->scene.instances;
    c->accel.vertsEdited = false;
    c->accel.built = true;
    c->accel.buildInfo.refit = kind;
    c->accel.msRefit = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->accel.buildInfo.ms_refit = c->accel.msRefit;
    c->accel.refits++;
    return SKH_OK;
}
// (an update that fails leaves no hierarchy behind: the next call builds)
static skh_status update_in_place(skh_context* c, bool verts /* vertices may have changed: the triangle tree is refitted */, bool moved /* instance transforms changed */,
                                  const std::vector<float>& w2o /* 12 per instance (invert_affine of the current table); may be empty when !moved */, uint32_t kind /* build_info.refit */)
{
    const skh_status s = update_stages(c, verts, moved, w2o, kind);
    if (s != SKH_OK)
        touched(c, skh_stale::IN_FAILED_UPDATE);
    return s;
}

// skh_refit_accel (round 6): offered for what a real bake is -- every mesh instance baked to world space (no top level: the world-only kernels) and nothing but
// the vertices / control points changed since the build; anything else falls back to the full rebuild, and the build info says which happened.
skh_status skh_refit_accel(skh_context* c)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    // (curves: control points and radii may have changed -- skh_set_curves with the built sets' table and vertex counts --; their tree is refitted the same way)
    const bool curvesOk = c->scene.curves.empty() ? c->accel.nSubBuilt == 0 : (c->accel.curveRefitReady && c->scene.curveSig == c->accel.builtCurveSig);
    const bool sameInstances = c->scene.instances.size() == c->accel.builtInstances.size() &&
                               (c->scene.instances.empty() || memcmp(c->scene.instances.data(), c->accel.builtInstances.data(), sizeof(skh_instance) * c->scene.instances.size()) == 0);
    const bool can = c->accel.refitReady && c->accel.updateReady && c->scene.geomSig == c->accel.builtGeomSig && c->scene.nVerts == c->accel.builtNVerts && c->accel.tlasRoot == SKH_REF_INVALID && curvesOk &&
                     sameInstances && (c->accel.triNumNodes > 0 || c->accel.segNumNodes > 0);
    c->accel.buildInfo.refit = 0;
    if (!can)
        return skh_build_accel(c, c->accel.lastBuildFlags);
    return update_in_place(c, true, false, std::vector<float>(), 1u);
}

// What keeps skh_update_accel from updating in place (nullptr: nothing).  Fills w2o (invert_affine of the new table) and whether any transform moved.
static const char* update_blocker(const skh_context* c, const skh_instance* in, uint32_t n, std::vector<float>& w2o, bool& moved)
{
    static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    moved = false;
    if (!c->accel.refitReady || !c->accel.updateReady)
        return "no build since the context was created or an option changed";
    if (c->scene.geomSig != c->accel.builtGeomSig || c->scene.nVerts != c->accel.builtNVerts)
        return "another mesh table or index buffer";
    if (!(c->scene.curves.empty() ? c->accel.nSubBuilt == 0 : (c->accel.curveRefitReady && c->scene.curveSig == c->accel.builtCurveSig)))
        return "another curve-set table or vertex counts, or the segment-node curve build";
    if (c->opt.tlasOpen > 1)
        return "tlas_open > 1 (opened TLAS leaves are BLAS subtrees)";
    if (n != c->accel.builtInstances.size())
        return "another instance count";
    w2o.resize(12 * (size_t)std::max(1u, n));
    for (uint32_t i = 0; i < n; ++i)
    {
        const skh_instance &a = in[i], &b = c->accel.builtInstances[i];
        if (a.type != b.type || a.geom_id != b.geom_id || a.material_id != b.material_id || a.light_id != b.light_id)
            return "an instance's type, geom_id, material_id or light_id";
        if (invert_affine(a.transform, &w2o[12 * (size_t)i]) != (c->accel.builtInvOk[i] != 0))
            return "a transform that became singular, or stopped being singular";
        moved = moved || memcmp(a.transform, b.transform, sizeof(a.transform)) != 0;
    }
    // decisions the build took from the transforms: which world-curve entry sits under a bit-exact identity (SKH_REF_CURVEROOT_IDENT), which curve instances share one
    for (uint32_t k = 0; k < c->accel.numWorldCurves; ++k)
    {
        const uint32_t i = c->accel.worldCurveInst[k];
        if ((memcmp(in[i].transform, kIdentity, sizeof(kIdentity)) == 0) != (memcmp(c->accel.builtInstances[i].transform, kIdentity, sizeof(kIdentity)) == 0))
            return "a world-curve entry that left or reached the identity transform";
    }
    for (const std::vector<uint32_t>& grp : c->accel.builtMergedGroups)
        for (uint32_t i : grp)
            if (memcmp(in[i].transform, in[grp[0]].transform, sizeof(in[i].transform)) != 0)
                return "a merged curve group whose members no longer share one transform";
    return nullptr;
}

skh_status skh_update_accel(skh_context* c, const skh_instance* instances, uint32_t n_instances)
{
    if (!c || (n_instances && !instances))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    const skh_instance* in = instances ? instances : c->scene.instances.data();
    const uint32_t n = instances ? n_instances : (uint32_t)c->scene.instances.size();
    std::vector<float> w2o;
    bool moved = false;
    const char* why = update_blocker(c, in, n, w2o, moved);
    c->accel.buildInfo.refit = 0;
    if (why)
    {
        if (getenv("SKH_DEBUG"))
            fprintf(stderr, "[skh] skh_update_accel: full build (%s)\n", why);
        skh_status s = instances ? skh_set_instances(c, instances, n_instances) : SKH_OK;
        return s != SKH_OK ? s : skh_build_accel(c, c->accel.lastBuildFlags);
    }
    if (instances)
    {
        touched(c, skh_stale::IN_UPDATED_INSTANCES);
        // (the table replaces whatever skh_set_instances set since the build -- which may have had another count: n is the built count here)
        c->scene.instances.assign(instances, instances + n);
        c->scene.nInstances = n;
        const skh_status s = dev_upload(c, c->scene.dInstances, instances, sizeof(skh_instance) * (size_t)n);
        if (s != SKH_OK)
        {
            touched(c, skh_stale::IN_FAILED_UPDATE);
            return s;
        }
    }
    return update_in_place(c, c->accel.vertsEdited, moved, w2o, 2u);
}

skh_status skh_get_baked(skh_context* c, uint8_t* flags, uint32_t n_instances, uint32_t* out_baked_instances, uint32_t* out_baked_triangles)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (!c->accel.built)
    {
        const skh_status s = skh_build_accel(c, SKH_BUILD_LBVH);
        if (s != SKH_OK)
            return s;
    }
    const bool on = true;
    if (flags)
        for (uint32_t i = 0; i < n_instances; ++i)
            flags[i] = (on && i < c->scene.nInstances && i < c->accel.baked.size()) ? c->accel.baked[i] : 0;
    if (out_baked_instances)
        *out_baked_instances = on ? c->accel.nBakedInst : 0u;
    if (out_baked_triangles)
        *out_baked_triangles = on ? c->accel.nBakedTris : 0u;
    return SKH_OK;
}
