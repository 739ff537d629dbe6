// The march step of render_persist at a leaf (rt_core.cuh:241-270) + the choice of the next step's restart node.
// Included into the kernel's loop body; expects in scope: rs, w (the leaf's
// word), slot, active, s_dst, (RTO_DEPTH: s_acc,) stack, stack_g, step_size, sigma_thresh, G, SPP, WIDE, kStackInRegs (compile time:
// the ancestor stack is the two registers stk0 / stk1), regstack (the same, possibly a run-time value).
                    RTO_DBG_AT(2)
                    // (WIDE: a wide entry, or a grid entry of the wide image, carries its leaf's level)
                    // rs.pos is 2^24 * clamp(cen + t * dir) of this very t (kPos24; computed when the previous step picked its
                    // restart node): cube_sz below is 2^(level + 1 - 24), inv_cube the reference's 2^-(level + 1)
                    uint32_t lvl_bits;  // level << 23
                    if constexpr (WIDE)
                        lvl_bits = w & kWideLevelMask;  // (a wide entry, or a grid entry of the wide image, carries its leaf's level there)
                    else
                        lvl_bits = (uint32_t)rs.prev_lvl << 23;
                    [[maybe_unused]] const int lvl = WIDE ? (int)(lvl_bits >> 23) : rs.prev_lvl;  // (only the stack forms of the restart read it)
                    const float cube_sz = __uint_as_float(lvl_bits + ((uint32_t)(128 - 24) << 23));
                    const float inv_cube = __uint_as_float(((uint32_t)126 << 23) - lvl_bits);
                    // _dda_unit (rt_core.cuh:38-51) on the leaf-local point frac(pos * cube_sz)
                    // (x and y as packed pairs: v_pk_mul_f32 / v_pk_add_f32 are the same IEEE operations, two per issue)
                    typedef float f2 __attribute__((ext_vector_type(2)));
                    // max(t1, t2) with t1 = -p * invdir, t2 = t1 + invdir (rt_core.cuh:44-48): invdir > 0 gives t2 >= t1, so the
                    // maximum IS t1 + invdir; invdir < 0 gives t2 <= t1, so it is t1 = t1 + 0 (a zero's sign aside, which the
                    // sums below cannot observe).  One add per axis instead of an add and a max (round 3: the kernel is bound
                    // by instruction issue and v_max_f32 costs two issue slots, profiles/r3_valu_calibration.json).
                    // The 1e4 start of the reference's running minimum never survives: dir is a unit vector, so one axis has
                    // |invdir| <= sqrt(3) and its exit time is below 2.
                    const f2 ixy = {rs.invdir[0], rs.invdir[1]};
                    const f2 sxy = (f2){rs.pos[0], rs.pos[1]} * cube_sz;
                    const f2 bxy = -(f2){__builtin_amdgcn_fractf(sxy.x), __builtin_amdgcn_fractf(sxy.y)} * ixy;
                    const f2 axy = bxy + (f2){rs.exit_add[0], rs.exit_add[1]};
                    const float b2 = -__builtin_amdgcn_fractf(rs.pos[2] * cube_sz) * rs.invdir[2];
                    const float a2 = b2 + rs.exit_add[2];
                    const float tm = __builtin_fminf(__builtin_fminf(axy.x, axy.y), a2);
                    const float delta_t = tm * inv_cube + step_size;
                    const float sigma = half_bits_to_float((uint16_t)w);
                    if (sigma > sigma_thresh) {
                        RTO_DBG_AT(3)
                        const float delta = delta_t * rs.delta_scale * sigma;
                        const float reach = rs.src + delta;
                        if (reach >= rs.cur) {
                            RTO_DBG_AT(4)
                            uint32_t cnt = 0;
                            {
                                // (the column's address is formed here: a loop-strength-reduced copy of it held across the
                                //  kernel costs a VGPR that a 64-register build spills -- and reloads in this very branch)
                                // (an LDS-address-space pointer: laundering the generic one turns the reads below into
                                //  flat_load_dword -- found in the round-5 disassembly, in 58 % of the iterations)
                                const __attribute__((address_space(3))) float* col = (const __attribute__((address_space(3))) float*)s_dst;
                                asm volatile("" : "+v"(col));
                                do {
                                    ++cnt;
                                    ++rs.spp;
                                    rs.cur = col[rs.spp * 256];
                                } while (reach >= rs.cur);
                            }
                            // entry k of the ray goes to row k of its threshold column: thresholds 1..spp are consumed, and
                            // k < spp (every hit crosses at least one threshold; row 0 never held one).  The list leaves in one go
                            // when the ray has ended (flush_hits; one store per hit at the moment it happens wrote 3x the bytes)
                            s_dst[rs.nh * 256] = __uint_as_float(hit_pack<SPP>(slot, cnt));
#if RTO_DEPTH
                            {   // the hit's distance (include/rto.h "depth outputs"): rs.t is the step's own, unscaled in every form.
                                // Every product and the add rounded; the sum left to right from 0.f
                                const float d = rs.t * rs.delta_scale;
                                s_acc[0] = (rs.nh == 0u ? 0.f : s_acc[0]) + (float)cnt * d;
                                if (rs.nh == 0u) s_acc[256] = d;
                            }
#endif
                            ++rs.nh;
                            if (rs.spp == (uint32_t)SPP) rs.tmax = -1.f;  // the last threshold: the ray ends
                        }
                        rs.src = reach;
                    }
                    rs.t += delta_t;
                    active = rs.t < rs.tmax;
                    if (active)
                    {  // next position -> restart node (deepest ancestor shared with this step).  (Running this for rays that
                       // just ended as well -- one divergent branch less per iteration -- measured 3 % SLOWER in one box:
                       // the register allocator pays for the merged live ranges with a dozen copies.)
                        RTO_DBG_AT(5)
                        const f2 pxy = rs.cxy + (f2){rs.dir[0], rs.dir[1]} * rs.t;
                        rs.pos[0] = clamp_unit24(pxy.x);
                        rs.pos[1] = clamp_unit24(pxy.y);
                        rs.pos[2] = clamp_unit24(rs.cen[2] + rs.t * rs.dir[2]);
                        const uint32_t ix = (uint32_t)rs.pos[0];  // (the scaled position IS the fixed-point one: kPos24)
                        const uint32_t iy = (uint32_t)rs.pos[1];
                        const uint32_t iz = (uint32_t)rs.pos[2];
                        // (v_bitop3_b32 with the table of (a ^ b) | c: three instructions for the three XORs and two ORs)
                        uint32_t diff = ix ^ rs.pix;
                        diff = __builtin_amdgcn_bitop3_b32(iy, rs.piy, diff, 0xBE);
                        diff = __builtin_amdgcn_bitop3_b32(iz, rs.piz, diff, 0xBE);
                        rs.pix = ix;
                        rs.piy = iy;
                        rs.piz = iz;
                        if constexpr (WIDE && kStackInRegs) {
                            // Two pairs of levels below the grid at most: WHERE the ray is says what the leaf's level could add.
                            // A node's index bits are the wb bits per axis from bit woff on; while the bits ABOVE them are the
                            // same for both points the next point lies in the same node (the reference's "deepest common
                            // ancestor, capped at the leaf's level": a leaf found in a node of a pair has a level of that pair, so
                            // the cap never names a deeper node than the one the ray is in -- at the grid woff + wb = 24: it stays).
                            // Leaving: to the grid when a bit at or above 24 - G differs, else (from the second pair) to the first
                            // pair's node, the one register of the ancestor stack.  No v_ffbh, no level arithmetic: two shifts /
                            // compares and five selects.
                            const uint32_t above = diff >> (rs.woff + rs.wb);
                            const bool stay = above == 0u, to_grid = diff >= tgrid;
                            rs.node = to_grid ? 0u : (stay ? rs.node : stk0);
                            rs.woff = to_grid ? woff_grid_v : (stay ? rs.woff : woff_pair0_v);
                            rs.wb = to_grid ? g_vgpr : rs.wb;  // (constants held in VGPRs: a select cannot read them and its condition from SGPRs)
                        } else {
                        // deepest level whose cell still holds both points: leading equal bits of the 24-bit coordinates,
                        // capped at the leaf's level (v_ffbh_u32 returns -1 for diff = 0; as an unsigned number that
                        // loses the minimum as well)
                        uint32_t lead;
                        asm("v_ffbh_u32 %0, %1" : "=v"(lead) : "v"(diff));
                        const uint32_t mu = lead - 8u;
                        const int m = (int)(mu < (uint32_t)lvl ? mu : (uint32_t)lvl);
                        if constexpr (WIDE) {
                            if (m < G) {  // back to the grid: G bits per axis from bit 24 - G on
                                rs.node = 0u;
                                rs.woff = 24u - (uint32_t)G;
                                rs.wb = (uint32_t)G;
                            } else {  // the wide node that spans level m: two bits per axis from bit 22 - G - 2 p on
                                const uint32_t pr = (uint32_t)(m - G) >> 1;
                                if (regstack)
                                    rs.node = pr ? stk1 : stk0;
                                else
                                    rs.node = stack[pr * 256u];
                                rs.woff = (22u - (uint32_t)G) - 2u * pr;
                                rs.wb = 2u;
                            }
                        } else {
                            if (m < G) {
                                rs.node = kGridNext;
                            } else {
                                rs.node = stack_g[m * 256];
                                rs.prev_lvl = m;
                            }
                        }
                        }
                    }
