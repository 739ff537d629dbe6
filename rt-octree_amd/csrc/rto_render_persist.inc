// rto_render_persist.inc -- body of the batched traversal kernel, included by render_kernels.hip into render_persist and
// render_persist_layers (RTO_PERSIST_LAYERS defined to 1 around the include: a ray stops at its pixel of the depth layer, `layers`,
// rto_ctx_set_layers).  In scope: the kernel parameters and SPP, REFILL, WPS, WIDE, STACK.  (Switched by the preprocessor:
// render_persist's text and code are what they were before the layered kernel existed.)
// RTO_DEPTH defined to 1 as well (render_persist_depth, depth_kernels.hip): a ray also keeps the distance of its hits (rto_march_leaf.inc)
// in two more LDS rows -- the sum and the first hit's; the forms without the register stack park hoff / hnext in two further ones -- and stores depth and t_near of its pixel through `dout` (DepthOut, plane f =
// batch frame f) when its hit list leaves.  Pixels whose ray never flushes are the launcher's fill: (0, +inf).
    // queue[8 + 8k]: next ray of queue k's list (zeroed on the stream before the launch)
    // LDS: [max_depth+1-top_levels][256] ancestor stack | [SPP+1][256] sorted thresholds | (RTO_DEPTH: [2 or 4][256] hit distances, hand-off offsets |) frame table
    extern __shared__ uint32_t s_mem[];
    const int tid = threadIdx.x;
    uint32_t* stack = s_mem + tid;  // [level - G][256]
    // levels top_levels.. only.  STACK == 1 (ancestor stack in a register): two rows all the same -- they hold a ray's two
    // hand-off offsets (rs.hoff, rs.hnext: written at the set-up, read at the flush, dead weight in the march loop whose
    // 64-register budget the restart's constants need)
    const int stack_levels = STACK == 1 ? 2 : tree.max_depth + 1 - tree.top_levels;
    float* s_dst = reinterpret_cast<float*>(s_mem + (size_t)stack_levels * 256) + tid;
    // the cameras of the batch: {fx, fy, transform[12]} per frame = the head of a FrameDesc (56 of its 96 bytes: at 100 frames
    // per launch the table then leaves room for 8 workgroups per CU)
#if RTO_DEPTH
    // the ray's depth accumulators: row 0 the running sum of (float)cnt * d over its hits, row 1 its first hit's d.  Written and
    // read at hits only (rare next to node visits): no register of the march loop, whose budget the layered kernel has used up
    float* s_acc = s_dst + (SPP + 1) * 256;
    // (the forms whose ancestor stack lives in LDS rows park the ray's two hand-off offsets in two more: held in registers, as their
    //  siblings hold them, these forms grow their private segment -- they are at 64 registers without the depth code)
    constexpr int kDepthRows = STACK == 1 ? 2 : 4;
    uint32_t* const s_offs = STACK == 1 ? stack : reinterpret_cast<uint32_t*>(s_acc) + 512;
    float* s_cams = reinterpret_cast<float*>(s_mem + (size_t)(stack_levels + SPP + 1 + kDepthRows) * 256);
#else
    float* s_cams = reinterpret_cast<float*>(s_mem + (size_t)(stack_levels + SPP + 1) * 256);
#endif
    __shared__ int s_qstart[kMaxQueues + 1];
    __shared__ uint32_t s_qcount[kMaxQueues];  // live tile slots of each queue (queue_scan_kernel)
    static_assert(offsetof(FrameDesc, transform) == 8 && kCamFloats == 14, "s_cams copies the first 14 floats of a FrameDesc");
    for (int i = tid; i < fb.n * kCamFloats; i += 256) {  // device memory -> LDS
        const int f = i / kCamFloats;
        s_cams[i] = reinterpret_cast<const float*>(fb.f + f)[i - f * kCamFloats];
    }
#pragma unroll
    for (int k = 0; k <= kMaxQueues; ++k)
        if (tid == 64 + k) s_qstart[k] = fb.qstart[k];
#pragma unroll
    for (int k = 0; k < kMaxQueues; ++k)
        if (tid == 128 + k) s_qcount[k] = k < fb.n_queues ? fb.qcount[k] : 0u;
    __syncthreads();

    const int W = fb.width, H = fb.height;
    const uint32_t SIZE = (uint32_t)W * (uint32_t)H;
    const uint32_t hstride = hit_stride(SIZE);  // distance between consecutive entries of one pixel (behind the first)
    // the queue this wave draws from first: the one of the XCD it runs on (HW_REG_XCC_ID bits 3:0)
    const uint32_t n_queues = (uint32_t)fb.n_queues;
    uint32_t cur_q = n_queues > 1 ? ((uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) % n_queues) : 0u;
    uint32_t q_tried = 0;            // queues found empty so far (wave-uniform)
    uint32_t res_off = 0;            // list offset of the queue the reservoir was drawn from (wave-uniform)

    // Loop-invariant scalars pinned in SGPRs: hipcc otherwise re-loads them from the kernarg segment inside the descent loop (an s_load +
    // lgkmcnt(0) round trip per level).
    typedef const __attribute__((address_space(1))) uint32_t* gptr_t;  // keep global_load (not flat_load)
    // WIDE: the two-level image and its top grid (host/tree_layout.cpp build_wide_image) instead of the one-level ones
    const uint32_t* nodew_p = WIDE ? tree.widew : tree.nodew;
    const uint2* topgrid_p = tree.topgrid;  // (WIDE: unused -- the grid cells are the first entries of the two-level image)
    const uint32_t* __restrict__ qlist = fb.qlist;
    float step_size = opt.step_size, sigma_thresh = opt.sigma_thresh;
    asm volatile("" : "+s"(nodew_p), "+s"(topgrid_p), "+s"(step_size), "+s"(sigma_thresh));
    const gptr_t nodew = (gptr_t)nodew_p;
    typedef unsigned int __attribute__((ext_vector_type(2))) u32x2;
    typedef const __attribute__((address_space(1))) u32x2* gptr2_t;
    const gptr2_t topgrid = (gptr2_t)topgrid_p;
    const int G = tree.top_levels;  // grid bits per axis; the LDS stack holds node levels G.. (entry 0 = level G)
    if (G == 0) stack[0] = 0u;      // no top grid: level 0 is the root
    // indexed by node level (only ever with levels >= G); WIDE: by the PAIR of levels (G + 2p, G + 2p + 1) a wide node spans
    uint32_t* const stack_g = WIDE ? stack : stack - G * 256;

#ifdef RTO_DBG_COUNTERS
    // per-branch occupancy of the march loop (tools/dbg_counters.py): for each branch, how many wave-level executions and
    // how many lanes took part.  0 iteration (any active lane), 1 descend, 2 leaf (march step), 3 sigma > thresh,
    // 4 hit (threshold crossed), 5 restart (ray goes on), 6 ray set-up (refill round), 7 grid lookups
    unsigned dbg_w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dbg_l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define RTO_DBG_AT(i)                                                                                          \
    {                                                                                                          \
        const unsigned long long m_ = __builtin_amdgcn_ballot_w64(true);                                      \
        ++dbg_l[i];                                                                                            \
        if ((tid & 63) == __ffsll((long long)m_) - 1) ++dbg_w[i];                                              \
    }
#else
#define RTO_DBG_AT(i) {}
#endif
    // Two pairs of levels below the grid at most (a tree of depth <= G + 4: the NeRF-synthetic PlenOctrees' 9-10 levels) and the
    // ancestor "stack" is two registers: the restart node then comes from a select, not from an LDS read on the path of
    // every iteration (-2 % in one box, profiles/r4_r_ab_regstack.txt).  Deeper trees keep the LDS rows.  (wave-uniform)
    uint32_t stk0 = 0u, stk1 = 0u;
    static_assert(WIDE || STACK == 0, "the register stack is for the two-level image");
    constexpr bool regstack = STACK == 1, kStackInRegs = regstack;
    uint32_t g_vgpr = (uint32_t)tree.top_levels;  // (rto_march_leaf.inc: the restart's `wb` select)
    asm volatile("" : "+v"(g_vgpr));
    // (the restart's selects, rto_march_leaf.inc: bit offsets of the grid and of the first pair below it, in VGPRs; the
    //  coordinate difference from which a ray is back at the grid, in an SGPR)
    uint32_t woff_grid_v = 24u - (uint32_t)tree.top_levels, woff_pair0_v = 22u - (uint32_t)tree.top_levels;
    uint32_t tgrid = 1u << (24 - tree.top_levels);
    asm volatile("" : "+v"(woff_grid_v), "+v"(woff_pair0_v), "+s"(tgrid));
#if !RTO_DEPTH  // (RTO_DEPTH: every form parks them, in s_offs)
    constexpr bool kOffsInLds = STACK == 1;
#endif
    RayState rs;
    // a lane marches a ray while rs.t < rs.tmax: that comparison IS the lane's state (an ended ray has t >= tmax or
    // tmax = -1), so the wave-level count of marching lanes is the ballot of one v_cmp instead of a loop-carried flag
    rs.t = 0.f;
    rs.tmax = -1.f;
    rs.nh = 0;
    bool drained = false;   // queue exhausted (wave-uniform)
    const uint32_t kChunk = chunk;           // rays per global dequeue (a multiple of the 64-ray tile)
    uint32_t res_next = 0, res_end = 0;      // the wave's private reservoir (wave-uniform)

    // Two nested loops (round 3): the OUTER one refills the wave, the INNER one marches until REFILL lanes are idle again.
    // The inner loop's back edge is one compare + population count + branch; with a single loop that re-decided "refill?"
    // at its top the compiler spent 14 scalar instructions per iteration on that decision -- and scalar instructions come
    // out of the same issue budget as the vector ones (profiles/r3_valu_calibration.json).
    for (;;) {
        {
            for (;;) {
                // (a finished ray needs no retiring: the stale threshold behind its last hit entry ends the list)
                if (drained) break;
                // ---- refill: hand the next queue entries to the idle lanes (ballot + prefix sum)
                const bool idle = !(rs.t < rs.tmax);
                const unsigned long long need = __builtin_amdgcn_ballot_w64(idle);
                const int n_need = __popcll(need);
                if (n_need < REFILL) break;
                // The wave draws rays from a private reservoir [res_next, res_end) and tops it up from
                // the global queue kChunk rays (kChunk/64 tiles) at a time: one device-scope atomic per
                // kChunk rays instead of one per refill (a single counter sustains only ~90 dequeues/us).
                if (res_next == res_end) {
                    for (;;) {  // own queue first, then the others in turn (wave-uniform)
                        const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane(s_qstart[cur_q]);
                        const uint32_t qtotal = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_qcount[cur_q]) * 64u;  // live rays
                        unsigned long long base = 0;
                        if ((tid & 63) == 0) base = atomicAdd(queue + 8 + 8 * cur_q, (unsigned long long)kChunk);
                        const uint32_t base32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                        if (base32 < qtotal) {  // a counter never exceeds qtotal + kChunk * waves: fits 32 bits
                            res_next = base32;
                            res_end = base32 + kChunk < qtotal ? base32 + kChunk : qtotal;
                            res_off = t0 * (uint32_t)fb.n;
                            break;
                        }
                        if (++q_tried >= n_queues) {
                            drained = true;
                            break;
                        }
                        cur_q = cur_q + 1 == n_queues ? 0u : cur_q + 1;
                    }
                    if (drained) break;
                }
                const uint32_t take = (uint32_t)n_need < res_end - res_next ? (uint32_t)n_need : res_end - res_next;
                const uint32_t first = res_next;
                res_next += take;
                if (idle && rs.nh) {  // the ended ray's hit list leaves in one go
#if RTO_DEPTH
                    depth_flush<SPP>(rs, s_offs, s_acc, dout, SIZE);  // (hoff / hnext back from their rows, depth and t_near stored)
#else
                    if constexpr (kOffsInLds) {
                        rs.hoff = stack[0];
                        rs.hnext = stack[256];
                    }
#endif
                    flush_hits<SPP, WIDE>(rs, tree, hits, s_dst, hstride, !tree.rec_by_entry);
                }
                if (idle) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                    const uint32_t r = first + rank;
                    // ray r of the queue: lane (r & 63) of the live tile slot qlist[.. + (r >> 6)] = {frame, tile y, tile x}
                    // (the lists hold marked tiles only: every ray handed out can meet density or at least crosses near it)
                    const uint32_t entry = rank < take ? qlist[res_off + (r >> 6)] : 0u;
                    const int frame = (int)(entry >> 20);
                    const int x = (int)(entry & 1023u) * 8 + (int)(r & 7u);  // (Z-order inside the tile was tried: no fewer L1 accesses)
                    const int y = (int)((entry >> 10) & 1023u) * 8 + (int)((r >> 3) & 7u);
                    if (rank < take && x < W && y < H) {
                        RTO_DBG_AT(6)
                        const float* fd = s_cams + frame * kCamFloats;
                        // (round 5: what the set-up derives from launch constants -- 0.5 W, bbox +- 1e-6 in double, the NDC factors --
                        //  is derived HERE: left alone the compiler hoists those values out of the kernel's loops into ~12 VGPRs and
                        //  spills them; the empty asm statements make the inputs opaque.  This was the kernel's whole private segment.)
                        int Wl = W, Hl = H;
                        OptDev o2 = opt;
                        TreeDev t2 = tree;
                        asm volatile("" : "+s"(Wl), "+s"(Hl));
#pragma unroll
                        for (int i = 0; i < 6; ++i) asm volatile("" : "+s"(o2.render_bbox[i]));
                        asm volatile("" : "+s"(t2.ndc_width), "+s"(t2.ndc_height), "+s"(t2.ndc_focal));
                        CamDev cam;
                        cam.width = Wl;
                        cam.height = Hl;
                        cam.fx = fd[0];
                        cam.fy = fd[1];
#pragma unroll
                        for (int i = 0; i < 12; ++i) cam.transform[i] = fd[2 + i];
                        float vdir[3];
                        ray_setup(x, y, cam, t2, rs.dir, vdir, rs.cen);
                        float tmin;
                        {   // where this pixel's next hit entry goes (hoff) and the one after it (hnext): hit_index
                            const uint32_t fbase = (uint32_t)frame * (uint32_t)SPP * SIZE, pixel = (uint32_t)(y * W + x);
                            rs.hoff = fbase + hit_index<SPP>(pixel, 0u, SIZE);
                            rs.hnext = fbase + hit_index<SPP>(pixel, SPP > 1 ? 1u : 0u, SIZE);
                        }
#if RTO_PERSIST_LAYERS
                        // the pixel's depth: plane `frame` of the launch's depth layer (frames x pixels < 2^32: the hand-off buffer's bound)
                        float tmax_bg = 1e9f;
                        if (layers.depth) tmax_bg = as_global(layers.depth)[(uint32_t)frame * SIZE + (uint32_t)(y * W + x)];
                        // (a depth <= 0 or NaN: not traced, as a degenerate ray of rto_launch_rays -- the ray ends like one that misses the box)
                        if (ray_is_live(tmax_bg, rs.dir, rs.cen) && ray_enter(t2, o2, rs.dir, rs.cen, tmax_bg, rs.invdir, rs.delta_scale, tmin, rs.tmax)) {
#else
                        if (ray_enter(t2, o2, rs.dir, rs.cen, 1e9f, rs.invdir, rs.delta_scale, tmin, rs.tmax)) {
#endif
                            // sorted thresholds of this pixel (sample_kernel left them in the hand-off
                            // buffer, where the ray's hit list will overwrite them)
                            rs.cur = __uint_as_float(hits[rs.hoff]);
                            const uint32_t* tp = hits + rs.hnext;
#if RTO_DEPTH
                            s_offs[0] = rs.hoff;  // (parked until the ray's flush)
                            s_offs[256] = rs.hnext;
#else
                            if constexpr (kOffsInLds) {  // (parked until the ray's flush)
                                stack[0] = rs.hoff;
                                stack[256] = rs.hnext;
                            }
#endif
#pragma unroll
                            for (int i = 1; i < SPP; ++i) s_dst[i * 256] = __uint_as_float(tp[(uint32_t)(i - 1) * hstride]);
                            s_dst[SPP * 256] = 3.402823466e+38f;
                            rs.spp = 0;
                            rs.src = 0;
                            rs.t = tmin;
                            float k24 = kPos24;  // (an SGPR operand: as a literal the compiler parks it in a VGPR pair across the kernel)
                            asm volatile("" : "+s"(k24));
#pragma unroll
                            for (int i = 0; i < 3; ++i) {  // (from here on the ray's origin and direction are the scaled ones: kPos24)
                                rs.cen[i] *= k24;
                                rs.dir[i] *= k24;
                            }
                            rs.cxy.x = rs.cen[0];
                            rs.cxy.y = rs.cen[1];
#pragma unroll
                            for (int i = 0; i < 3; ++i) rs.exit_add[i] = rs.invdir[i] > 0.f ? rs.invdir[i] : 0.f;
                            rs.pix = rs.piy = rs.piz = 0;
                            rs.prev_lvl = 0;
                            {  // locate the first position: fixed-point coordinates + first node
#pragma unroll
                                for (int i = 0; i < 3; ++i) rs.pos[i] = clamp_unit24(rs.cen[i] + rs.t * rs.dir[i]);
                                rs.pix = (uint32_t)rs.pos[0];
                                rs.piy = (uint32_t)rs.pos[1];
                                rs.piz = (uint32_t)rs.pos[2];
                                rs.node = WIDE ? 0u : (G > 0 ? kGridNext : 0u);
                                rs.woff = 24u - (uint32_t)G;
                                rs.wb = (uint32_t)G;
                            }
                        } else {
                            rs.tmax = -1.f;  // missed the box (ray_enter wrote a tmax that the stale t might undercut)
                        }
                    }
                }
            }
        }
        bool active = rs.t < rs.tmax;
        if (__builtin_amdgcn_ballot_w64(active) == 0ULL) {
            if (drained) break;
            continue;  // (every ray of the round missed the volume)
        }
        // once the queues are empty there is nothing to refill with: march until the last ray ends
        const int exit_at = drained ? 0 : 64 - REFILL;
        int n_active;
        do {
        {
            // ---- one node visit for every active lane
            if (active) {
                RTO_DBG_AT(0)
                uint32_t slot, w;
                if constexpr (WIDE) {
                    // Round 4: ONE array holds the top grid and the two-level ("wide") nodes below it (host/tree_layout.cpp
                    // build_wide_image), so a node visit is ONE uniform load: entry = ((node << b | x bits) << b | y bits) << b |
                    // z bits, b bits per axis from bit rs.woff on -- (node, b, woff) = (0, G, 24 - G) at the grid,
                    // (node number, 2, 22 - G - 2 p) at the wide node of the levels (G + 2p, G + 2p + 1).  v_bfe_u32 and
                    // v_lshl_or_b32 take the per-lane widths: no grid / node case split, no second address, no branch pair
                    // around two loads (the one-level walk below spends 19 VALU + 7 SALU where this spends 10 VALU).
                    const uint32_t b = rs.wb;
                    slot = (rs.node << b) | __builtin_amdgcn_ubfe(rs.pix, rs.woff, b);
                    slot = (slot << b) | __builtin_amdgcn_ubfe(rs.piy, rs.woff, b);
                    slot = (slot << b) | __builtin_amdgcn_ubfe(rs.piz, rs.woff, b);
                    if (rs.node == 0u) { RTO_DBG_AT(7) }
#ifdef RTO_STUB_LOADS
                    {   // calibration build (tools/calibrate_valu.sh): the gather replaced by a hash of its address
                        const uint32_t hsh = slot * 0x9E3779B1u;
                        const uint32_t sg = (hsh & 0x600u) ? 0u : 0x4D00u;
                        if (rs.node == 0u) {
                            const uint32_t glv = 2u + (hsh >> 30);
                            w = (glv == 5u && (hsh & 0x100u)) ? ((hsh >> 8) & 0xffffu) | 1u : (kLeafTag | glv << kWideLevelShift | sg);
                        } else {  // two pairs below the grid (levels G .. G + 3), leaves at either level of a pair
                            const uint32_t lv = 22u - rs.woff + ((hsh >> 27) & 1u);
                            w = (rs.woff == 22u - (uint32_t)G && (hsh >> 29) < 5u) ? ((hsh >> 8) & 0xffffu) | 1u : (kLeafTag | lv << kWideLevelShift | sg);
                        }
                    }
#else
                    // (through the L1: non-temporal loads cost 15-50 %.  The byte offset as a 32-bit value -- the image has < 2^29
                    //  entries -- lets the load take its base from SGPRs and one VGPR of offset: no 64-bit address pair, no register
                    //  pinned to zero for its high half)
                    w = *(gptr_t)((const __attribute__((address_space(1))) char*)nodew + (uint32_t)(slot << 2));
#endif
                    if ((int32_t)w >= -(1 << 30)) {  // internal: two levels down (from the grid: into the level-G node)
                        RTO_DBG_AT(1)
                        rs.node = w;
                        if (regstack) {
                            // two pairs at most: the ancestor "stack" is ONE register, the node of the first pair.  (The second
                            // pair's node needs none: a restart inside the second pair happens at a leaf of that very node --
                            // the ray stays in rs.node.)
                            const bool first = rs.woff == 24u - (uint32_t)G;
                            stk0 = first ? w : stk0;
                        } else
                            stack[(((24u - (uint32_t)G) - rs.woff) >> 1) * 256u] = w;  // row p + 1 of the pair it spans (grid: row 0)
                        rs.woff -= 2u;
                        rs.wb = 2u;
                    }
                }
                if constexpr (!WIDE) {
                const bool grid = rs.node == kGridNext;
                const uint32_t gs = 24u - (uint32_t)G;
                const uint32_t key = (((rs.pix >> gs) << G | (rs.piy >> gs)) << G) | (rs.piz >> gs);
                const uint32_t sh = 23u - (uint32_t)rs.prev_lvl;
                slot = (rs.node << 1) | __builtin_amdgcn_ubfe(rs.pix, sh, 1u);  // node * 8 + child digit,
                slot = (slot << 1) | __builtin_amdgcn_ubfe(rs.piy, sh, 1u);       // three v_lshl_or
                slot = (slot << 1) | __builtin_amdgcn_ubfe(rs.piz, sh, 1u);
                // Both addresses exist in registers before either load is issued.  Left to itself the compiler sinks each
                // address computation into its branch, and when a temporary of the second branch lands in the register the
                // first branch's load is still writing, it has to put an s_waitcnt vmcnt(0) between the two loads -- the
                // iteration then pays two memory latencies back to back (measured: 8.16 instead of 7.16 ms per 100
                // frames from a one-instruction difference elsewhere in the kernel that renumbered the registers).
                gptr_t pn = nodew + slot;
                gptr2_t pg = topgrid + key;
                asm volatile("" : "+v"(pn), "+v"(pg));
#ifdef RTO_STUB_LOADS
                // Calibration build only (tools/calibrate_valu.sh): both gathers replaced by a hash of their address -- a
                // procedural stand-in for the tree with the same loop, the same divergence and no memory latency, to measure
                // what the loop body sustains in VALU instructions per clock at 1..8 waves per SIMD.  Never shipped.
                if (grid) {
                    const uint32_t hsh = key * 0x9E3779B1u;
                    const uint32_t glv = 2u + (hsh >> 30);
                    slot = (key << 3) & kGridSlotMask;
                    const uint32_t sg = (hsh & 0x600u) ? 0u : 0x4D00u;
                    rs.prev_lvl = (int)glv;
                    rs.node = slot >> 3;
                    w = (glv == 5u && (hsh & 0x100u)) ? 1u : (kLeafTag | sg);
                } else {
                    const uint32_t hsh = slot * 0x9E3779B1u;
                    const uint32_t sg = (hsh & 0x600u) ? 0u : 0x4D00u;
                    w = (rs.prev_lvl < 9 && (hsh >> 29) < 3u) ? 1u : (kLeafTag | sg);
                }
#else
                if (grid) {  // the iteration's one load: 8 bytes of the top grid ...
                    const u32x2 e = *pg;  // (through the L1 as well: non-temporal costs 15 %)
                    slot = e.x & kGridSlotMask;
                    rs.prev_lvl = (int)(e.x >> kGridSlotBits);
                    rs.node = slot >> 3;
                    w = e.y;
                } else {  // ... or 4 bytes of the traversal image
                    w = *pn;  // (through the L1: a non-temporal load here costs 50 %)
                }
#endif
                if (grid) { RTO_DBG_AT(7) }
                if ((int32_t)w >= -(1 << 30)) {  // internal: one level down
                    RTO_DBG_AT(1)
                    rs.node += w;
                    ++rs.prev_lvl;
                    stack_g[rs.prev_lvl * 256] = rs.node;
                }
                }  // (!WIDE)
                if ((int32_t)w < -(1 << 30)) {  // leaf: the march step (rt_core.cuh:241-270)
#include "rto_march_leaf.inc"
                }
            }
        }
            active = rs.t < rs.tmax;
            {
                const unsigned long long am = __builtin_amdgcn_ballot_w64(active);
                asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n_active) : "s"(am) : "scc");
            }
        } while (n_active > exit_at);
    }
    if (rs.nh) {  // rays that ended after the last refill round
#if RTO_DEPTH
        depth_flush<SPP>(rs, s_offs, s_acc, dout, SIZE);
#else
        if constexpr (kOffsInLds) {
            rs.hoff = stack[0];
            rs.hnext = stack[256];
        }
#endif
        flush_hits<SPP, WIDE>(rs, tree, hits, s_dst, hstride, !tree.rec_by_entry);
    }
#ifdef RTO_DBG_COUNTERS
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // queue words 1..7 / 9..15 are padding of the queue counters: wave counts, lane counts
        const int wi = i == 0 ? 16 + 1 : i, li = i == 0 ? 16 + 2 : 8 + i;
        if (dbg_w[i]) atomicAdd(queue + wi, (unsigned long long)dbg_w[i]);
        if (dbg_l[i]) atomicAdd(queue + li, (unsigned long long)dbg_l[i]);
    }
#endif
