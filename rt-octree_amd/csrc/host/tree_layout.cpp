// tree_layout.cpp -- see tree_layout.h.  No HIP in this unit.
#include "host/tree_layout.h"

#include <cmath>
#include <cstring>

#include "host/n3tree_host.h"
#include "rto_tree_bits.h"

namespace rto {

float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    uint32_t bits;
    if (exp == 0) {
        if (man == 0) {
            bits = sign;
        } else {  // subnormal: renormalise
            int e = -1;
            uint32_t m = man;
            do {
                ++e;
                m <<= 1;
            } while (!(m & 0x400u));
            bits = sign | (uint32_t)(127 - 15 - e) << 23 | (m & 0x3ffu) << 13;
        }
    } else if (exp == 31) {
        bits = sign | 0x7f800000u | man << 13;
    } else {
        bits = sign | (exp + 127 - 15) << 23 | man << 13;
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

bool culling_cells(const int32_t* child, int64_t capacity, const float scale[3], const float offset[3], const uint16_t* sigma,
                   size_t stride, std::vector<float>& out, std::vector<float>* cubes) {
    auto density = [&](int64_t sl) { return half_to_float(sigma[(size_t)sl * stride]); };
    std::vector<uint8_t> lvl((size_t)capacity, 255), has((size_t)capacity, 0);
    std::vector<uint32_t> cx((size_t)capacity, 0), cy((size_t)capacity, 0), cz((size_t)capacity, 0);
    // per node and axis: the bounds [lo, hi] of the subtree's dense leaves as fractions of the NODE'S OWN cube, in units of
    // 2^-31 of its edge.  A slot is half the edge (2^30), a child's bounds are halved on the way up: every value is a multiple
    // of 2^(30 - levels below) with at most 30 levels below, so the shifts drop no bit; and 0 <= lo < hi <= 2^31 whatever
    // child[] holds -- relative bounds cannot leave their cell even where a damaged child[] gives a node two parents.
    constexpr uint32_t kHalf = 1u << 30;
    std::vector<uint32_t> blo((size_t)capacity * 3, 0), bhi((size_t)capacity * 3, 0);
    lvl[0] = 0;
    for (int64_t n = 0; n < capacity; ++n) {  // top-down: level and integer cell coordinates of every reachable node
        if (lvl[(size_t)n] == 255) continue;
        for (int s = 0; s < 8; ++s) {
            const int32_t c = child[n * 8 + s];
            if (c == 0) continue;
            const int64_t t = n + c;
            if (t <= n || t >= capacity || lvl[(size_t)n] >= 30) return false;
            lvl[(size_t)t] = (uint8_t)(lvl[(size_t)n] + 1);
            cx[(size_t)t] = cx[(size_t)n] * 2 + ((s >> 2) & 1);  // slot = x * 4 + y * 2 + z (n3tree_query.hpp:26-33)
            cy[(size_t)t] = cy[(size_t)n] * 2 + ((s >> 1) & 1);
            cz[(size_t)t] = cz[(size_t)n] * 2 + (s & 1);
        }
    }
    for (int64_t n = capacity - 1; n >= 0; --n) {  // bottom-up: does the subtree hold a leaf of positive density, and where?
        if (lvl[(size_t)n] == 255) continue;
        uint8_t h = 0;
        uint32_t lo[3] = {2 * kHalf, 2 * kHalf, 2 * kHalf}, hi[3] = {0, 0, 0};
        for (int s = 0; s < 8; ++s) {
            const int32_t c = child[n * 8 + s];
            if (!(c ? has[(size_t)(n + c)] : (uint8_t)(density(n * 8 + s) > 0.f))) continue;
            h = 1;
            const uint32_t bit[3] = {(uint32_t)(s >> 2) & 1u, (uint32_t)(s >> 1) & 1u, (uint32_t)s & 1u};
            for (int i = 0; i < 3; ++i) {  // a dense leaf slot is its whole half of the edge, a child brings its own bounds
                const uint32_t l = bit[i] * kHalf + (c ? blo[(size_t)(n + c) * 3 + i] >> 1 : 0u);
                const uint32_t u = bit[i] * kHalf + (c ? bhi[(size_t)(n + c) * 3 + i] >> 1 : kHalf);
                lo[i] = l < lo[i] ? l : lo[i];
                hi[i] = u > hi[i] ? u : hi[i];
            }
        }
        has[(size_t)n] = h;
        for (int i = 0; i < 3 && h; ++i) blo[(size_t)n * 3 + i] = lo[i], bhi[(size_t)n * 3 + i] = hi[i];
    }
    out.clear();
    if (cubes) cubes->clear();
    const float margin = 1e-4f;  // tree units: far above the float error of cen + t * dir (~1e-6), far below a cell
    // (it pads the bounds as it pads a cube: they are a union of leaf cubes, and a sample point inside a dense leaf lies inside
    //  that leaf's cube)
    for (int64_t n = 0; n < capacity; ++n) {
        if (lvl[(size_t)n] == 255 || !has[(size_t)n]) continue;
        const int ls = lvl[(size_t)n] + 1;  // the node's child slots are cubes of size 2^-ls
        if (ls > kOccLevel) continue;  // inside a cube emitted above
        for (int s = 0; s < 8; ++s) {
            const int32_t c = child[n * 8 + s];
            const bool emit = c ? (ls == kOccLevel && has[(size_t)(n + c)]) : density(n * 8 + s) > 0.f;
            if (!emit) continue;
            const double size = std::ldexp(1.0, -ls);
            const uint32_t q[3] = {cx[(size_t)n] * 2 + ((s >> 2) & 1), cy[(size_t)n] * 2 + ((s >> 1) & 1), cz[(size_t)n] * 2 + (s & 1)};
            // a record: {world centre, 0} {half-extents in TREE units, 0}.  The padded half-extents (a multiple of the finest
            // leaf + the margin: exact to 1e-9 as floats); the kernel divides by |TreeDev::scale| per axis for the world
            // half-widths of the box
            float box[8] = {0.f}, cube[8] = {0.f};
            for (int i = 0; i < 3; ++i) {
                // a leaf slot is the cube; below a node of the culling level, the bounds of its subtree's dense leaves
                const double l = c ? std::ldexp((double)blo[(size_t)(n + c) * 3 + i], -31) : 0.0;
                const double u = c ? std::ldexp((double)bhi[(size_t)(n + c) * 3 + i], -31) : 1.0;
                box[i] = (float)(((q[i] + 0.5 * (l + u)) * size - offset[i]) / scale[i]);
                box[4 + i] = (float)(0.5 * (u - l) * size + margin);
                cube[i] = (float)(((q[i] + 0.5) * size - offset[i]) / scale[i]);
                cube[4 + i] = (float)(0.5 * size + margin);
            }            out.insert(out.end(), box, box + 8);
            if (cubes) cubes->insert(cubes->end(), cube, cube + 8);
        }
    }
    return true;
}

std::vector<int64_t> bfs_order(const int32_t* child, int64_t capacity, int64_t N3) {
    std::vector<int64_t> order;
    order.reserve((size_t)capacity);
    std::vector<uint8_t> seen((size_t)capacity, 0);
    order.push_back(0);
    seen[0] = 1;
    for (size_t h = 0; h < order.size(); ++h) {
        const int64_t o = order[h];
        for (int64_t s = 0; s < N3; ++s) {
            const int32_t c = child[o * N3 + s];
            if (c == 0) continue;
            const int64_t t = o + c;  // in range: tree_max_depth validated every offset
            if (!seen[(size_t)t]) {
                seen[(size_t)t] = 1;
                order.push_back(t);
            }
        }
    }
    for (int64_t o = 0; o < capacity; ++o)
        if (!seen[(size_t)o]) order.push_back(o);
    return order;
}

void relay_tree(const std::vector<int64_t>& order, const int32_t* child, const uint16_t* data, int64_t capacity, int64_t N3,
                int data_dim, const HostTree* quant, Relaid& out) {
    std::vector<int64_t> new_of_old((size_t)capacity);
    for (int64_t n = 0; n < capacity; ++n) new_of_old[(size_t)order[(size_t)n]] = n;
    out.child.resize((size_t)(capacity * N3));
    for (int64_t n = 0; n < capacity; ++n) {
        const int64_t o = order[(size_t)n];
        for (int64_t s = 0; s < N3; ++s) {
            const int32_t c = child[o * N3 + s];
            out.child[(size_t)(n * N3 + s)] = c ? (int32_t)(new_of_old[(size_t)(o + c)] - n) : 0;
        }
    }
    auto gather = [&](const uint16_t* src, size_t per_slot, uint16_t* dst) {  // [capacity*N3][per_slot]
        const size_t node_elems = (size_t)N3 * per_slot;
        for (int64_t n = 0; n < capacity; ++n)
            std::memcpy(dst + (size_t)n * node_elems, src + (size_t)order[(size_t)n] * node_elems, node_elems * sizeof(uint16_t));
    };
    if (data) {
        out.data.resize((size_t)(capacity * N3) * (size_t)data_dim);
        gather(data, (size_t)data_dim, out.data.data());
    }
    if (quant) {
        const size_t ns = (size_t)(capacity * N3);
        const int nq = quant->n_basis - quant->n_retain, nr = quant->n_retain;
        out.q_sigma.resize(ns);
        gather(quant->q_sigma, 1, out.q_sigma.data());
        out.q_map.resize((size_t)nq * ns);
        for (int j = 0; j < nq; ++j) gather(quant->q_map + (size_t)j * ns, 1, out.q_map.data() + (size_t)j * ns);  // plane by plane
        out.q_retained.resize((size_t)nr * ns * 3);
        for (int j = 0; j < nr; ++j) gather(quant->q_retained + (size_t)j * ns * 3, 3, out.q_retained.data() + (size_t)j * ns * 3);
    }
}

bool build_wide_image(const int32_t* child, int64_t capacity, int G, const uint16_t* sigma, size_t stride,
                      WideImage& out) {
    // node ranges of the levels (the tree is stored breadth-first: a level's nodes are contiguous)
    std::vector<int64_t> start(1, 0), end(1, 1);
    for (int l = 0; l < 64; ++l) {
        int64_t hi = end[(size_t)l];
        for (int64_t n = start[(size_t)l]; n < end[(size_t)l]; ++n)
            for (int s = 0; s < 8; ++s) {
                const int32_t c = child[n * 8 + s];
                if (c != 0 && n + c + 1 > hi) hi = n + c + 1;
                if (c != 0 && n + c < end[(size_t)l]) return false;  // not breadth-first after all
            }
        if (hi == end[(size_t)l]) break;  // no children: the last level
        start.push_back(end[(size_t)l]);
        end.push_back(hi);
        if (hi > capacity) return false;
    }
    const int n_levels = (int)start.size();
    if (n_levels > 25 || G >= n_levels) return false;
    std::vector<int64_t> pair_base;  // first wide node of pair p
    int64_t n_wide = 0;
    for (int L = G; L < n_levels; L += 2) {
        pair_base.push_back(n_wide);
        n_wide += end[(size_t)L] - start[(size_t)L];
    }
    const int64_t grid_cells = int64_t(1) << (3 * G);
    const int64_t grid_nodes = (grid_cells + 63) / 64;
    if ((grid_nodes + n_wide) * 64 >= (int64_t(1) << kGridSlotBits)) return false;
    out.n_wide = (uint32_t)n_wide;
    out.grid_nodes = (uint32_t)grid_nodes;
    out.widew.assign((size_t)(grid_nodes + n_wide) * 64, kLeafTag);  // (padding reads as an empty leaf of level 0; never indexed)
    out.worig.assign((size_t)n_wide, 0u);
    auto leafw = [&](int level, int64_t slot) { return kLeafTag | ((uint32_t)level << kWideLevelShift) | (uint32_t)sigma[(size_t)slot * stride]; };
    auto entry = [](int a, int b) {  // child digits (x most significant) at level L and L + 1 -> position in the wide node
        const int x2 = ((a >> 2) & 1) << 1 | ((b >> 2) & 1), y2 = ((a >> 1) & 1) << 1 | ((b >> 1) & 1), z2 = (a & 1) << 1 | (b & 1);
        return x2 << 4 | y2 << 2 | z2;
    };
    for (size_t p = 0; p < pair_base.size(); ++p) {
        const int L = G + 2 * (int)p;
        for (int64_t N = start[(size_t)L]; N < end[(size_t)L]; ++N) {
            const int64_t wn = pair_base[p] + (N - start[(size_t)L]);
            out.worig[(size_t)wn] = (uint32_t)N;
            uint32_t* w = out.widew.data() + (size_t)(grid_nodes + wn) * 64;
            for (int a = 0; a < 8; ++a) {
                const int32_t c = child[N * 8 + a];
                if (c == 0) {
                    const uint32_t lw = leafw(L, N * 8 + a);
                    for (int b = 0; b < 8; ++b) w[entry(a, b)] = lw;
                    continue;
                }
                const int64_t C = N + c;
                for (int b = 0; b < 8; ++b) {
                    const int32_t c2 = child[C * 8 + b];
                    if (c2 == 0) {
                        w[entry(a, b)] = leafw(L + 1, C * 8 + b);
                    } else {
                        const int64_t D = C + c2;  // level L + 2: the first level of the next pair
                        if (L + 2 >= n_levels || D < start[(size_t)L + 2] || D >= end[(size_t)L + 2]) return false;
                        w[entry(a, b)] = (uint32_t)(grid_nodes + pair_base[p + 1] + (D - start[(size_t)L + 2]));
                    }
                }
            }
        }
    }
    // the top grid in the same terms (see build_topgrid_kernel): cell -> where its root path over levels 0..G-1 ends
    {
        const uint32_t mask = (1u << G) - 1u;
        out.gslot.assign((size_t)grid_cells, 0u);
        for (uint32_t key = 0; key < (uint32_t)grid_cells; ++key) {
            if (G == 0) {  // no grid levels: the one cell is the whole volume, below it the root's wide node
                out.widew[0] = (uint32_t)grid_nodes;
                break;
            }
            const uint32_t cx = key >> (2 * G), cy = (key >> G) & mask, cz = key & mask;
            int64_t node = 0, slot = 0;
            int32_t c = 0;
            int lvl = 0;
            for (;;) {
                const int sh = G - 1 - lvl;
                const uint32_t ci = (((cx >> sh) & 1u) << 2) | (((cy >> sh) & 1u) << 1) | ((cz >> sh) & 1u);
                slot = node * 8 + ci;
                c = child[slot];
                if (c == 0 || lvl == G - 1) break;
                node += c;
                ++lvl;
            }
            if (c == 0) {
                out.widew[key] = leafw(lvl, slot);
                out.gslot[key] = (uint32_t)slot;
            } else {  // internal at level G - 1: its child is a level-G node = a wide node of pair 0
                const int64_t D = node + c;
                if (D < start[(size_t)G] || D >= end[(size_t)G]) return false;
                out.widew[key] = (uint32_t)(grid_nodes + (D - start[(size_t)G]));
            }
        }
    }
    return true;
}

void wide_image_lookup(const WideImage& wi, const int32_t* child, int G, const uint32_t* points, int64_t n, int32_t* out_level,
                       int64_t* out_slot, uint16_t* out_sigma) {
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t ix = points[i * 3], iy = points[i * 3 + 1], iz = points[i * 3 + 2];
        // render_persist's walk: (node, off) = (0, 24 - G) at the grid, (node number, 22 - G - 2 p) at pair p below;
        // entry = ((node << b | x bits) << b | y bits) << b | z bits with b = node ? 2 : G bits per axis from bit `off` on
        uint32_t w = 0, u = 0, node = 0, off = 24u - (uint32_t)G;
        for (;;) {
            const uint32_t b = node ? 2u : (uint32_t)G, m = (1u << b) - 1u;
            u = (((node << b | ((ix >> off) & m)) << b | ((iy >> off) & m)) << b) | ((iz >> off) & m);
            w = wi.widew[u];
            if (nodew_is_leaf(w)) break;
            node = w;  // internal: the node two levels down (from the grid: the level-G node's)
            off -= 2u;
        }
        // hit index -> leaf slot (rto_tree_device.h wide_to_slot)
        int64_t slot;
        const uint32_t pad = wi.grid_nodes * 64u;
        if (u < pad) {
            slot = (int64_t)wi.gslot[u];
        } else {
            const uint32_t v = u - pad, wn = v >> 6, x2 = (v >> 4) & 3u, y2 = (v >> 2) & 3u, z2 = v & 3u;
            const uint32_t a = (x2 >> 1) << 2 | (y2 >> 1) << 1 | (z2 >> 1), b = (x2 & 1u) << 2 | (y2 & 1u) << 1 | (z2 & 1u);
            const int64_t N = wi.worig[wn];
            slot = child[N * 8 + a] == 0 ? N * 8 + a : (N + child[N * 8 + a]) * 8 + b;
        }
        out_level[i] = (int32_t)((w >> kWideLevelShift) & 31u);
        out_slot[i] = slot;
        out_sigma[i] = (uint16_t)(w & 0xffffu);
    }
}

}  // namespace rto
