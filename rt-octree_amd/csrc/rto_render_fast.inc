// rto_render_fast.inc -- body of the single-frame fast kernel, included by frame_kernels.hip into render_fast (LOBES = 0: SH and
// RGBA trees), render_fast_lobes (LOBES = kFmtSG / kFmtASG) and render_rays (RTO_FAST_RAYS defined to 1 around the include: the
// rays of rto_launch_rays instead of a camera's pixels) and render_fast_layers (RTO_FAST_LAYERS defined to 1: a camera's pixels,
// each ray stopped at its pixel of the depth layer and composited over its pixel of the colour layer -- `layers`, rto_ctx_set_layers).
// RTO_DEPTH defined to 1 as well (render_rays_depth, render_fast_layers_depth): the ray also keeps the distance of its hits -- d =
// t * delta_scale at the top of the march step that collides -- and stores depth and t_near through `dout` (DepthOut,
// include/rto.h "depth outputs"): two multiplies, an add and a select per hit, no load, two registers, two 4-byte stores.
// In scope: the kernel parameters and SPP, STATS, WIDE, STACK, LOBES.
// (The ray source is switched by the preprocessor, not by if constexpr: the frame kernels' text -- and so their code -- is
// exactly what it was before the ray kernel existed.)
    extern __shared__ uint32_t s_stack[];  // [max_depth][256] ancestor node indices, level-major

#if RTO_FAST_RAYS
    const int tid = threadIdx.x;
    const uint32_t ray = ray_index(rays, blockIdx.x, tid);
    if (ray >= rays.n) return;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
#if RTO_DEPTH
    float dsum = 0.f, tnear = __builtin_inff();
#endif
    float dir[3], vdir[3], cen[3], invdir[3], tmax_bg, bg[3];
    const bool live = ray_from_batch(rays, ray, tree, opt.background_brightness, dir, vdir, cen, tmax_bg, bg);  // (false: degenerate)
#else
    int tx, ty;
    if (!block_tile(tm, blockIdx.x, tx, ty)) return;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int x = tx * kTileW + wave * 8 + (lane & 7);
    const int y = ty * kTileH + (lane >> 3);
    if (x >= cam.width || y >= cam.height) return;
    const int64_t SIZE = (int64_t)cam.width * cam.height;
    const int idx = y * cam.width + x;

    float out[4] = {0.f, 0.f, 0.f, 0.f};
#if RTO_DEPTH
    float dsum = 0.f, tnear = __builtin_inff();
#endif
#if RTO_FAST_LAYERS
    float bg[3];
    layer_backdrop(layers, (uint32_t)idx, opt.background_brightness, bg);
#endif
    if (!STATS && fo.cull_marks) {  // (wave-uniform: a wave is one 8x8 tile)
        const uint32_t t = (uint32_t)(y >> 3) * ((uint32_t)(cam.width + 7) >> 3) + (uint32_t)(x >> 3);
        if (!(((fo.cull_marks[t >> 5] >> (t & 31u)) | fo.cull_marks[fo.cull_mask_words - 1]) & 1u)) {
#if RTO_FAST_LAYERS
            write_pixel_over(fo, SIZE, idx, bg, out);  // no ray of this tile meets density, whatever its depth: the backdrop
#if RTO_DEPTH
            write_depth(dout, (uint32_t)idx, dsum, tnear);  // (... and no hit: 0, +inf)
#endif
#else
            write_pixel(fo, SIZE, idx, opt.background_brightness, out);  // no ray of this tile meets density: background
#endif
            return;
        }
    }
    float dir[3], vdir[3], cen[3], invdir[3];
    ray_setup(x, y, cam, tree, dir, vdir, cen);
#if RTO_FAST_LAYERS
    const float tmax_bg = layers.depth ? layers.depth[idx] : 1e9f;
    const bool live = ray_is_live(tmax_bg, dir, cen);  // (false: not traced, as a degenerate ray of rto_launch_rays)
#endif
#endif
    float delta_scale, tmin, tmax;
    unsigned long long st_steps = 0, st_levels = 0, st_hits = 0, st_inbox = 0, st_grid = 0, st_words = 0, st_wide = 0;
#if RTO_FAST_RAYS
    if (live && ray_enter(tree, opt, dir, cen, tmax_bg, invdir, delta_scale, tmin, tmax)) {
        Pcg32 rng = rng_base;
        pcg_advance_tab(rng, ray * (uint32_t)SPP, jump);  // (the host keeps n * SPP < 2^32)
#elif RTO_FAST_LAYERS
    if (live && ray_enter(tree, opt, dir, cen, tmax_bg, invdir, delta_scale, tmin, tmax)) {
        Pcg32 rng = rng_base;
        pcg_advance_tab(rng, (uint32_t)(idx * SPP), jump);
#else
    if (ray_enter(tree, opt, dir, cen, 1e9f, invdir, delta_scale, tmin, tmax)) {
        if (STATS) st_inbox = 1;
        Pcg32 rng = rng_base;
        pcg_advance_tab(rng, (uint32_t)(idx * SPP), jump);
#endif

        // thresholds, ascending; dst[0] is always the next one to cross (consumed ones shift out)
        float dst[SPP + 1];
#pragma unroll
        for (int n = 0; n < SPP; ++n) {
            float tv = -det_log_one_minus(pcg_next_float(rng));
#pragma unroll
            for (int i = 0; i < n; ++i) {  // static-index insertion: same sorted array
                const float lo = __builtin_fminf(dst[i], tv), hi = __builtin_fmaxf(dst[i], tv);  // (see sample_kernel)
                dst[i] = lo;
                tv = hi;
            }
            dst[n] = tv;
        }
        dst[SPP] = 3.402823466e+38f;

        uint32_t hits[SPP];
#pragma unroll
        for (int i = 0; i < SPP; ++i) hits[i] = 0;
        uint32_t spp = 0, sh_nums = 0;
        float src = 0;
        float t = tmin;

        uint32_t pix = 0, piy = 0, piz = 0;
        int prev_lvl = 0;
        uint32_t* stack = s_stack + tid;
        const int G = tree.top_levels;  // 0: no top grid
        if (WIDE && G == 0) stack[0] = 0u;
        uint32_t stk0 = 0u, stk1 = 0u;
        const bool regstack = WIDE && (tree.max_depth - G + 1) / 2 <= 2;  // (uniform) pairs of levels below the grid
        const float exit_add[3] = {invdir[0] > 0.f ? invdir[0] : 0.f, invdir[1] > 0.f ? invdir[1] : 0.f, invdir[2] > 0.f ? invdir[2] : 0.f};
        static_assert(STACK == 0 || (WIDE && !STATS), "the register-stack restart is for the two-level image");
        // STACK == 1: the node / bit offset / bits per axis the NEXT step starts from (render_persist's rs.node, rs.woff, rs.wb)
        uint32_t cnode = 0u, coff = 24u - (uint32_t)G, cb = (uint32_t)G;
        const uint32_t tgrid = 1u << (24 - G);
        if constexpr (STACK == 1) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // (kPos24)
                cen[i] *= kPos24;
                dir[i] *= kPos24;
            }
        }

        while (t < tmax) {
            // (round 5: the arithmetic forms of the batched kernel's march step -- one v_med3 per clamp, v_fract, the exit
            //  time as t1 + (invdir > 0 ? invdir : 0), no 1e4 start of the minimum: see rto_march_leaf.inc for why each is the
            //  same number -- a lone frame waits for the DEPENDENT chain of its longest ray, a third of which is this arithmetic:
            //  0.307 -> 0.295 ms per lone 800x800 SPP-6 frame, profiles/r5_w_ab_fast.txt)
            float pos[3];
            uint32_t ix, iy, iz;
            if constexpr (STACK == 1) {
#pragma unroll
                for (int i = 0; i < 3; ++i) pos[i] = clamp_unit24(cen[i] + t * dir[i]);
                ix = (uint32_t)pos[0];
                iy = (uint32_t)pos[1];
                iz = (uint32_t)pos[2];
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) pos[i] = clamp_unit(cen[i] + t * dir[i]);
                ix = (uint32_t)(pos[0] * 16777216.f);
                iy = (uint32_t)(pos[1] * 16777216.f);
                iz = (uint32_t)(pos[2] * 16777216.f);
            }
            // levels whose child digit is unchanged since the previous step
            const uint32_t diff = (ix ^ pix) | (iy ^ piy) | (iz ^ piz);
            int lvl = 0;
            if constexpr (STACK != 1) {
                lvl = __clz((int)diff) - 8;
                lvl = lvl < prev_lvl ? lvl : prev_lvl;
            }
            uint32_t node, w, slot;
            bool have_w = false;
            if constexpr (STACK == 1) {
                // (see rto_march_leaf.inc: the same node while the bits above its index bits are unchanged; back to the grid when a
                //  bit at or above 24 - G differs; else, from the second pair, the first pair's node)
                const bool stay = (diff >> (coff + cb)) == 0u, to_grid = diff >= tgrid;
                node = to_grid ? 0u : (stay ? cnode : stk0);
                uint32_t off = to_grid ? 24u - (uint32_t)G : (stay ? coff : 22u - (uint32_t)G);
                uint32_t b = to_grid ? (uint32_t)G : cb;
                for (;;) {
                    slot = (node << b) | __builtin_amdgcn_ubfe(ix, off, b);
                    slot = (slot << b) | __builtin_amdgcn_ubfe(iy, off, b);
                    slot = (slot << b) | __builtin_amdgcn_ubfe(iz, off, b);
                    w = *(const uint32_t*)((const char*)tree.widew + (uint32_t)(slot << 2));  // (< 2^29 entries: a 32-bit byte offset)
                    if (nodew_is_leaf(w)) break;
                    stk0 = off == 24u - (uint32_t)G ? w : stk0;  // (the first pair's node: the one ancestor a later step may need)
                    node = w;  // the wide node two levels down
                    off -= 2u;
                    b = 2u;
                }
                cnode = node;
                coff = off;
                cb = b;
                (void)have_w;
                (void)stk1;
            } else if constexpr (WIDE) {
                // the two-level image (host/tree_layout.cpp build_wide_image; round 4): one load per TWO levels below the grid -- a lone
                // frame waits for the dependent-load chains of its longest rays, and this shortens every one of them
                // (node, off): (0, 24 - G) = the top grid, whose cells are indexed by G bits per axis; else the wide node of the
                // pair (G + 2 pr, G + 2 pr + 1), two bits per axis from bit 22 - G - 2 pr on.  One array holds both.
                // With two pairs of levels below the grid at most (regstack: a tree of depth <= G + 4) the ancestor stack is two
                // registers: no LDS round trip on the dependent chain of a step.
                int pr = -1;
                node = 0u;
                if (lvl >= G) {
                    pr = (lvl - G) >> 1;
                    node = regstack ? (pr ? stk1 : stk0) : stack[pr * 256];
                    if (node == 0u) pr = -1;  // (no grid levels, first step: the stack still holds the 0 it was given)
                }
                for (;;) {
                    const uint32_t b = node ? 2u : (uint32_t)G, msk = (1u << b) - 1u;
                    const uint32_t off = node ? (uint32_t)(22 - G - 2 * pr) : 24u - (uint32_t)G;
                    slot = (((node << b | ((ix >> off) & msk)) << b | ((iy >> off) & msk)) << b) | ((iz >> off) & msk);
                    w = *(const uint32_t*)((const char*)tree.widew + (uint32_t)(slot << 2));  // (< 2^29 entries: a 32-bit byte offset)
                    if (nodew_is_leaf(w)) break;
                    node = w;  // the wide node two levels down
                    ++pr;
                    if (regstack) {
                        stk0 = pr == 0 ? node : stk0;
                        stk1 = pr == 0 ? stk1 : node;
                    } else {
                        stack[pr * 256] = node;
                    }
                }
                (void)have_w;
                lvl = (int)((w >> kWideLevelShift) & 31u);  // a leaf word of the wide image carries its level
            } else {
            if (lvl < G) {
                // restart above the shortcut levels: ONE 8-byte lookup replaces the walk over node levels
                // 0..G-1 (a chain of dependent loads -- what a lone frame's long rays wait for) and
                // already carries the word of the slot where that walk ends
                const uint32_t gs = 24u - (uint32_t)G;
                const uint32_t key = (((ix >> gs) << G | (iy >> gs)) << G) | (iz >> gs);
                const uint2 e = tree.topgrid[key];
                slot = e.x & kGridSlotMask;
                lvl = (int)(e.x >> kGridSlotBits);
                node = slot >> 3;
                w = e.y;
                have_w = true;
                if (STATS) ++st_grid;
            } else {
                node = lvl ? stack[lvl * 256] : 0u;
            }
            int st_pair = -1;  // STATS: the pair of levels whose wide node the two-level image would have loaded last
            for (;;) {
                if (!have_w) {
                    const int sh = 23 - lvl;
                    const uint32_t ci = (((ix >> sh) & 1u) << 2) | (((iy >> sh) & 1u) << 1) | ((iz >> sh) & 1u);
                    slot = node * 8u + ci;
                    w = tree.nodew[slot];
                    if (STATS) {
                        ++st_words;
                        // render_persist on the two-level image loads ONE entry per pair of levels (G + 2p, G + 2p + 1)
                        const int pr = (lvl - G) >> 1;
                        if (pr != st_pair) ++st_wide;
                        st_pair = pr;
                    }
                }
                have_w = false;
                if (nodew_is_leaf(w)) break;
                node += w;  // two's complement add of the relative offset
                ++lvl;
                stack[lvl * 256] = node;
            }
            }
            pix = ix;
            piy = iy;
            piz = iz;
            prev_lvl = lvl;
            if (STATS) {
                ++st_steps;
                st_levels += (unsigned)(lvl + 1);
            }

            // cube_sz = 2^(lvl+1) and its reciprocal straight from exponent bits; x / 2^k == x * 2^-k
            // bit for bit (a pure exponent shift, or the same single rounding into the denormals)
            float cube_sz, inv_cube;
            if constexpr (STACK == 1) {  // (positions scaled by 2^24: 2^(level + 1 - 24); the level at the word's exponent bits)
                const uint32_t lvl_bits = w & kWideLevelMask;
                cube_sz = __uint_as_float(lvl_bits + ((uint32_t)(128 - 24) << 23));
                inv_cube = __uint_as_float(((uint32_t)126 << 23) - lvl_bits);
            } else {
                cube_sz = __uint_as_float((uint32_t)(128 + lvl) << 23);
                inv_cube = __uint_as_float((uint32_t)(126 - lvl) << 23);
            }
            float ex[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) ex[i] = -__builtin_amdgcn_fractf(pos[i] * cube_sz) * invdir[i] + exit_add[i];
            const float t_subcube = __builtin_fminf(__builtin_fminf(ex[0], ex[1]), ex[2]) * inv_cube;
            const float delta_t = t_subcube + opt.step_size;
            const float sigma = half_bits_to_float((uint16_t)(w & 0xffffu));
            if (sigma > opt.sigma_thresh) {
                const float delta = delta_t * delta_scale * sigma;
                if (src + delta >= dst[0]) {
                    uint32_t cnt = 0;
                    do {
                        ++cnt;
                        ++spp;
#pragma unroll
                        for (int i = 0; i < SPP; ++i) dst[i] = dst[i + 1];
                    } while (src + delta >= dst[0]);
#if RTO_DEPTH
                    {  // (t: the step's own, unscaled in every form -- STACK == 1 scales cen and dir, not t)
                        const float d = t * delta_scale;
                        dsum += (float)cnt * d;
                        tnear = sh_nums == 0u ? d : tnear;
                    }
#endif
                    // (the counting instantiation walks the one-level image; a tree whose records follow the two-level image's
                    //  entries needs the leaf's entry there: found by that image's walk -- this kernel is never timed)
                    const uint32_t h = hit_pack<SPP>(!WIDE && tree.rec_by_entry ? wide_entry_of(tree, ix, iy, iz) : slot, cnt);
#pragma unroll
                    for (int i = 0; i < SPP; ++i) hits[i] = (i == (int)sh_nums) ? h : hits[i];
                    ++sh_nums;
                    if (spp == SPP) break;
                }
                src += delta;
            }
            t += delta_t;
        }

        if (STATS) st_hits = sh_nums;
#if RTO_DEPTH
        dsum *= 1.0f / SPP;
#endif
#if RTO_DEPTH && RTO_FAST_RAYS
        if (sh_nums != 0 && rays.out) {  // (uniform: a call that asks for no colour shades nothing)
#else
        if (sh_nums != 0) {
#endif
            float basis_fn[RTO_BASIS_MAX_DEV];
            ray_basis<LOBES>(tree, opt, vdir, basis_fn);
            constexpr bool kLobes = LOBES != 0;  // (an SG / ASG tree's records are laid out as an SH tree's of the same data_dim)
#pragma unroll
            for (int i = 0; i < SPP; ++i) {
                if (i < (int)sh_nums) {
                    uint32_t slot = hit_slot<SPP>(hits[i]);
                    if constexpr (WIDE)
                        if (!tree.rec_by_entry) slot = wide_to_slot(tree, slot);  // hit index of the wide image -> the leaf's slot
                    const float cnt = (float)hit_count<SPP>(hits[i]);
                    if ((kLobes || tree.format == 1) && tree.data_dim == 28)
                        shade_leaf_packed<28>(tree, slot, basis_fn, cnt, out);
                    else if ((kLobes || tree.format == 1) && tree.data_dim == 49)
                        shade_leaf_packed<49>(tree, slot, basis_fn, cnt, out);
                    else if ((kLobes || tree.format == 1) && tree.data_dim == 76)
                        shade_leaf_packed<76>(tree, slot, basis_fn, cnt, out);
                    else
                        shade_leaf(tree, tree.data + (uint64_t)slot * tree.data_dim, basis_fn, cnt, out);
                }
            }
            constexpr float INV_SPP = 1.0f / SPP;
            out[0] *= INV_SPP;
            out[1] *= INV_SPP;
            out[2] *= INV_SPP;
            out[3] *= INV_SPP;
        }
    }
#if RTO_FAST_RAYS && RTO_DEPTH
    if (rays.out) write_ray(rays, ray, bg, out);
    write_depth(dout, ray, dsum, tnear);
    (void)st_steps, (void)st_levels, (void)st_hits, (void)st_inbox, (void)st_grid, (void)st_words, (void)st_wide;  // (STATS only)
#elif RTO_FAST_RAYS
    write_ray(rays, ray, bg, out);
    (void)st_steps, (void)st_levels, (void)st_hits, (void)st_inbox, (void)st_grid, (void)st_words, (void)st_wide;  // (STATS only)
#elif RTO_FAST_LAYERS
    write_pixel_over(fo, SIZE, idx, bg, out);
#if RTO_DEPTH
    write_depth(dout, (uint32_t)idx, dsum, tnear);
#endif
    (void)st_steps, (void)st_levels, (void)st_hits, (void)st_inbox, (void)st_grid, (void)st_words, (void)st_wide;  // (STATS only)
#else
    write_pixel(fo, SIZE, idx, opt.background_brightness, out);
    if (STATS) {  // order as orc_stats: rays, rays_in_box, steps, levels, hit_leaves, hit_rays
        atomicAdd(fo.stats + 0, 1ULL);
        atomicAdd(fo.stats + 1, st_inbox);
        atomicAdd(fo.stats + 2, st_steps);
        atomicAdd(fo.stats + 3, st_levels);
        atomicAdd(fo.stats + 4, st_hits);
        atomicAdd(fo.stats + 5, st_hits ? 1ULL : 0ULL);
        // the same ray as the batched path sees it: marched only if its 8x8 tile is marked (mark_tiles_kernel); one
        // top-grid entry or one traversal-image word per node visit is exactly what render_persist loads (same restart rule)
        bool marched = true;
        if (fo.stat_marks) {
            const uint32_t t = (uint32_t)(y >> 3) * ((uint32_t)(cam.width + 7) >> 3) + (uint32_t)(x >> 3);
            marched = ((fo.stat_marks[t >> 5] >> (t & 31u)) | fo.stat_marks[fo.stat_mask_words - 1]) & 1u;
        }
        if (marched) {
            atomicAdd(fo.stats + 6, 1ULL);
            atomicAdd(fo.stats + 7, st_steps);
            atomicAdd(fo.stats + 8, st_grid);
            atomicAdd(fo.stats + 9, st_words);
            atomicAdd(fo.stats + 10, st_hits);
            atomicAdd(fo.stats + 11, st_inbox);
            atomicAdd(fo.stats + 12, st_wide);
        }
    }
#endif
