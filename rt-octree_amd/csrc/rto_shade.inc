// rto_shade.inc -- body of the batched path's shading kernel, included by shade_kernels.hip into shade_kernel and
// shade_kernel_layers (RTO_SHADE_LAYERS defined to 1 around the include: a pixel -- live or culled -- is composited over its pixel
// of the colour layer, `layers`, rto_ctx_set_layers, where it is stored).  In scope: the kernel parameters and SPP, P, MODE, LOBES.
// (Switched by the preprocessor: shade_kernel's text and code are what they were before the layered kernel existed.)
    __shared__ uint32_t s_h[kShadeWaves][kShadeCap];       // packed hit entry
    __shared__ uint16_t s_q[kShadeWaves][kShadeCap];       // its pixel, relative to the wave's first pixel
    __shared__ float s_c[kShadeWaves][3 * kShadeCap];      // its contribution, [channel][entry]
    const int W = fb.width, H = fb.height;
    const int64_t SIZE = (int64_t)W * H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#ifdef RTO_DBG_COUNTERS
    unsigned long long ph[8];
    for (int i = 0; i < 8; ++i) ph[i] = 0;
    RTO_SHADE_STAMP(0)
#endif
    // Workgroup -> (pixel block, frame), XCD-aware: workgroups go round-robin over the 8 XCDs, so id & 7 picks the XCD, and the L2 is
    // per XCD.  Rounds 2-5 put the same 128-pixel block of ALL frames of the batch on one XCD, frame after frame, hoping that
    // neighbouring poses hit the same leaves there; the counters never agreed (L2 hit 15 %, as with frame-major order): an orbiting
    // camera moves a leaf SIDEWAYS by ten or twenty pixels per frame -- out of its block after a few frames, but not out of its rows.
    // Round 6: BANDS of 8 rows.  Band b of all frames runs on XCD b & 7, frame after frame, a band's blocks side by side: L2 hit
    // 0.15 -> 0.28, FETCH 4.25 -> 3.56 GB per 100 C2 frames, 1.335 -> 1.298 ms (C4 6.75 -> 6.23, C5 0.985 -> 0.936); bands of 4 / 16 /
    // 32 rows: 1.306 / 1.315 / 1.43 (profiles/r6_y_ab_shade_bands*.txt, r6_y_pmc_shade_bands.txt).  RTO_SHADE_BAND_ROWS=0: the old order.
    const uint32_t bid = blockIdx.x, q = bid >> 3;
#if RTO_SHADE_BAND_ROWS > 0
    const uint32_t cpb = shade_blocks_per_band(W, 64 * kShadeWaves * P), per_band = cpb * (uint32_t)fb.n;
    const uint32_t bi = q / per_band, rem = q - bi * per_band;
    const uint32_t frame = rem / cpb;
    const uint32_t pblock = (bi * 8u + (bid & 7u)) * cpb + (rem - frame * cpb);
#else
    const uint32_t frame = q % (uint32_t)fb.n;
    const uint32_t pblock = (q / (uint32_t)fb.n) * 8u + (bid & 7u);
#endif
    const int64_t wave_px0 = ((int64_t)pblock * kShadeWaves + wv) * (64 * P);
    if (wave_px0 >= SIZE) return;  // wave-uniform
    const FrameDesc& fd = fb.f[frame];  // block-uniform index: scalar loads
    // (the frame's hand-off lists: from the launch's base, not from the frame table -- a wave's first loads then depend on its
    //  kernel arguments only; a shading wave spends a fifth of its life before its hit lists have arrived, profiles/r6_d_shade_phases.txt)
    const RTO_GLOBAL uint32_t* const fhits = as_global(hits0) + (size_t)frame * (size_t)SPP * (size_t)SIZE;

    // ---- each lane: the hit lists of its P pixels (pixel p*64 + lane of the wave: coalesced)
    uint32_t h[P][SPP];
    uint32_t n[P];
    uint32_t mine = 0, live_bits = 0;  // bit p: pixel p of this lane lies in a marked tile
    // A pixel of a culled tile has no hit list (nobody wrote one: sample_kernel, render_persist): it is read off the tile
    // marks, a few hundred cached words per frame, instead of 4 * SPP bytes per pixel of stale memory -- two thirds of the
    // pixels of the bench scene.  (x, y) of the wave's first pixel by one wave-uniform division, the lanes' by carries.
    const uint32_t* fmask = fb.tile_mask ? fb.tile_mask + (size_t)frame * fb.mask_words : nullptr;
    const uint32_t keep_all = fmask ? fmask[fb.mask_words - 1] & 1u : 1u;
    const int tiles_x = (W + 7) >> 3;
    const int wy0 = (int)(wave_px0 / W), wx0 = (int)(wave_px0 - (int64_t)wy0 * W);
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int64_t idx = wave_px0 + p * 64 + lane;
        n[p] = 0;
        bool live = idx < SIZE;
        if (live && fmask) {  // (the mark word is requested before the frame's keep-all flag is back: no dependent second trip)
            int x = wx0 + p * 64 + lane, y = wy0;
            while (x >= W) {
                x -= W;
                ++y;
            }
            const uint32_t t = (uint32_t)((y >> 3) * tiles_x + (x >> 3));
            live = (((fmask[t >> 5] >> (t & 31u)) | keep_all) & 1u) != 0u;
        }
        live_bits |= live ? 1u << p : 0u;
        if (live) {
            bool open = true;
            // the first entry from its dense plane, the run behind it (fetched eagerly: fetching the run only for a pixel whose
            // first entry is valid saves 20 bytes per empty pixel and costs a dependent round trip per wave, 2.03 vs 1.95 ms)
            uint32_t raw[SPP];
            raw[0] = fhits[idx];
            const RTO_GLOBAL uint32_t* hp = fhits + SIZE + idx * (SPP - 1);
#pragma unroll
            for (int i = 1; i < SPP; ++i) raw[i] = hp[i - 1];
#pragma unroll
            for (int i = 0; i < SPP; ++i) {
                open = open && (raw[i] & kHitValid) != 0u;
                h[p][i] = open ? raw[i] : 0u;
                n[p] += open ? 1u : 0u;
            }
        }
        mine += n[p];
    }
    // (sparse lean outputs: a wave whose pixels all lie in unmarked tiles -- two thirds of the bench scene's waves -- has nothing to
    //  shade and nothing to store)
    if (fb.lean == 2 && __builtin_amdgcn_ballot_w64(live_bits != 0u) == 0ULL) return;
    // ---- wave exclusive prefix sum -> each pixel's range in the compacted list
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const uint32_t total = __shfl(inc, 63, 64);
    RTO_SHADE_STAMP(1)  // tile marks + hit lists are here (the prefix sum consumed them)
    uint32_t start[P];
    {
        uint32_t sacc = inc - mine;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            start[p] = sacc;
            sacc += n[p];
        }
    }
    float out[P][4];
#pragma unroll
    for (int p = 0; p < P; ++p) out[p][0] = out[p][1] = out[p][2] = out[p][3] = 0.f;

    CamDev cam;
    cam.width = W;
    cam.height = H;
    cam.fx = fd.fx;
    cam.fy = fd.fy;
#pragma unroll
    for (int i = 0; i < 12; ++i) cam.transform[i] = fd.transform[i];

    for (uint32_t w0 = 0; w0 < total; w0 += kShadeCap) {  // wave-uniform
        // ---- pixel lanes publish the entries that fall into this window
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int i = 0; i < SPP; ++i) {
                const uint32_t pos = start[p] + i - w0;  // wraps to a huge value below the window
                if ((uint32_t)i < n[p] && pos < (uint32_t)kShadeCap) {
                    s_h[wv][pos] = h[p][i];
                    s_q[wv][pos] = (uint16_t)(p * 64 + lane);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- one entry per lane
        RTO_SHADE_STAMP(2)  // (last window's) entries published
        const uint32_t cnt_w = min(total - w0, (uint32_t)kShadeCap);
        for (uint32_t j = lane; j < cnt_w; j += 64) {
            const uint32_t he = s_h[wv][j];
            // the entry's pixel = pixel s_q of the wave's run, which starts at (wx0, wy0): carries instead of a 64-bit division
            // per entry (round 5: `idx % W`, `idx / W` on an int64 were ~150 of the ~690 instructions an entry cost)
            int x = wx0 + (int)s_q[wv][j], y = wy0;
            while (x >= W) {
                x -= W;
                ++y;
            }
            float dir[3], vdir[3], cen[3];
            ray_setup(x, y, cam, tree, dir, vdir, cen);  // only vdir is needed (rt_core.cuh:278)
            float basis_fn[RTO_BASIS_MAX_DEV];
            // (view direction + basis once per hit PIXEL, parked in LDS, removes ~200 of these ~430 instructions per entry and was
            //  built twice -- round 4 and round 6, tools/experiments/r6_shade_basis_table.patch -- and lost both times: 1.54 vs
            //  1.48 ms on C2, 1.24 vs 1.02 on C5: this arithmetic runs while the entry's record is in flight and costs nothing)
            if constexpr (LOBES != 0 && MODE > 0)  // SG / ASG tree, data_dim = MODE
                ray_basis_lobes<LOBES, (MODE - 1) / 3>(tree, opt, vdir, basis_fn);
            else if constexpr (MODE > 0)  // (the launcher picks MODE from the tree: SH, data_dim = MODE)
                ray_basis_sh<(MODE - 1) / 3>(opt, vdir, basis_fn);
            else if constexpr (MODE < 0)  // quantised SH tree, -MODE basis functions
                ray_basis_sh<-MODE>(opt, vdir, basis_fn);
            else
                ray_basis<LOBES>(tree, opt, vdir, basis_fn);
            float o[4];
            leaf_contrib<MODE>(tree, hit_slot<SPP>(he), basis_fn, (float)hit_count<SPP>(he), o);
            s_c[wv][j] = o[0];
            s_c[wv][kShadeCap + j] = o[1];
            s_c[wv][2 * kShadeCap + j] = o[2];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- pixel lanes add their entries up, in hit order
        RTO_SHADE_STAMP(3)  // (last window's) entries shaded
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int i = 0; i < SPP; ++i) {
                const uint32_t pos = start[p] + i - w0;
                if ((uint32_t)i < n[p] && pos < (uint32_t)kShadeCap) {
                    out[p][0] += s_c[wv][pos];
                    out[p][1] += s_c[wv][kShadeCap + pos];
                    out[p][2] += s_c[wv][2 * kShadeCap + pos];
                    out[p][3] += (float)hit_count<SPP>(h[p][i]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    RTO_SHADE_STAMP(4)  // sums done
    RTO_GLOBAL float* const g_aux = as_global(fd.aux);
    typedef float f4_t __attribute__((ext_vector_type(4)));  // (HIP's float4 has no assignment across address spaces)
    RTO_GLOBAL f4_t* const g_image = (RTO_GLOBAL f4_t*)as_global(fd.image);
    constexpr float INV_SPP = 1.0f / SPP;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int64_t idx = wave_px0 + p * 64 + lane;
        if (idx >= SIZE) continue;
        if (n[p]) {  // (a pixel without hits keeps its exact zeros, as before)
            out[p][0] *= INV_SPP;
            out[p][1] *= INV_SPP;
            out[p][2] *= INV_SPP;
            out[p][3] *= INV_SPP;
        }
        // volrend.cu:174-212 (write_pixel, through global-address-space pointers): background composite, then the 8 aux planes
        // and the RGBA32F image with alpha = 1 -- or, lean (block-uniform), the four values their consumers read in one store
#if RTO_SHADE_LAYERS
        // (volrend.cu:161-185 with offscreen = false: over the pixel's backdrop -- write_ray's arithmetic)
        float bg[3];
        layer_backdrop(layers, (uint32_t)frame * (uint32_t)SIZE + (uint32_t)idx, opt.background_brightness, bg);
        const float nalpha = 1.f - out[p][3];
        const float r = out[p][0] + bg[0] * nalpha, g = out[p][1] + bg[1] * nalpha, b = out[p][2] + bg[2] * nalpha, al = out[p][3];
#else
        const float remain = opt.background_brightness * (1.f - out[p][3]);
        const float r = out[p][0] + remain, g = out[p][1] + remain, b = out[p][2] + remain, al = out[p][3];
#endif
        if (fb.lean) {
            // (sparse, level 2: nothing for a pixel of an unmarked tile -- it is the background and its consumers know it)
            if (fb.lean == 1 || ((live_bits >> p) & 1u)) g_image[idx] = f4_t{r, g, b, al};
        } else {
            RTO_GLOBAL float* a = g_aux + idx;
            a[0] = r;
            a[SIZE] = g;
            a[2 * SIZE] = b;
            a[3 * SIZE] = al;
            a[4 * SIZE] = r * r;
            a[5 * SIZE] = g * g;
            a[6 * SIZE] = b * b;
            a[7 * SIZE] = al * al;
            g_image[idx] = f4_t{r, g, b, 1.0f};
        }
    }
#ifdef RTO_DBG_COUNTERS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have left
    RTO_SHADE_STAMP(5)
    if (lane == 0 && blockIdx.x * (uint32_t)kShadeWaves + (uint32_t)wv < (uint32_t)kShadeStampWaves) {
        unsigned long long* o = g_shade_phase + (size_t)(blockIdx.x * (uint32_t)kShadeWaves + (uint32_t)wv) * 8;
        for (int i = 0; i <= 5; ++i) o[i] = ph[i];
        o[6] = total;
        o[7] = 1;
    }
#endif
