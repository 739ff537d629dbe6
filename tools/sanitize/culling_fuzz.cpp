// culling_fuzz.cpp -- culling_cells (host/tree_layout.cpp) under AddressSanitizer + UBSan, a stand-alone program (CPU only; build
// + run: tools/sanitize/run_culling.sh).  Seeded random trees (depth 1 .. 12, breadth-first with unreachable spare nodes, random
// anisotropic off-centre frames, densities positive / zero / negative / NaN) held to what the tile marks rest on:
//   * cells and their cube form come in pairs, in the same order; a cube's half-extents are one value
//   * every box lies inside its cube (never outside its cell), and is the cube where the cell is a leaf
//   * every dense leaf, found here by an independent recursive walk, lies inside the box of the cell whose cube holds it, and
//     that box is tight: on each of its six faces lies a face of one of those leaves
// then the same trees with mutated `child` arrays (offsets out of range, backwards, onto shared or spare nodes): true or false,
// never a report, and where true every box still inside its cube.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "host/tree_layout.h"
#include "rto_tree_bits.h"

namespace {

constexpr double kMargin = 1e-4, kTol = 2e-6;  // culling_cells' margin; float rounding of a world centre brought back to tree units

struct Tree {
    std::vector<int32_t> child;
    std::vector<uint16_t> sigma;  // [capacity * 8 * stride]
    size_t stride = 1;
    int64_t capacity = 0;
    float scale[3], offset[3];
};

Tree random_tree(std::mt19937_64& rng) {
    Tree t;
    const int depth = 1 + (int)(rng() % 12);
    const int64_t budget = 1 + (int64_t)(rng() % 600);
    const int split = 20 + (int)(rng() % 60);  // per cent of the slots of a node that get a child
    std::vector<int> level(1, 0);
    t.child.assign(8, 0);
    for (int64_t n = 0; n < (int64_t)level.size(); ++n)  // breadth-first: children are appended behind every node so far
        for (int s = 0; s < 8; ++s) {
            if (level[(size_t)n] + 1 >= depth || (int64_t)level.size() >= budget || (int)(rng() % 100) >= split) continue;
            t.child[(size_t)n * 8 + s] = (int32_t)((int64_t)level.size() - n);
            level.push_back(level[(size_t)n] + 1);
            t.child.resize(level.size() * 8, 0);
        }
    const int64_t spare = (int64_t)(rng() % 4);
    t.capacity = (int64_t)level.size() + spare;
    t.child.resize((size_t)t.capacity * 8, 0);
    for (size_t i = level.size() * 8; i < t.child.size(); ++i) t.child[i] = (int32_t)(rng() % 5) - 2;  // garbage nobody reaches
    t.stride = 1 + (size_t)(rng() % 3);
    t.sigma.resize((size_t)t.capacity * 8 * t.stride);
    static const uint16_t kinds[] = {0x0000, 0x8000, 0x3c00, 0x6dc0, 0x0001, 0xbc00, 0x7e00, 0x7c00};  // 0 -0 1 5888 tiny -1 NaN inf
    const int dense = 5 + (int)(rng() % 60);
    for (auto& v : t.sigma) v = (int)(rng() % 100) < dense ? kinds[2 + rng() % 6] : kinds[rng() % 2];
    for (int i = 0; i < 3; ++i) {
        t.scale[i] = (float)(0.05 + (double)(rng() % 1000) / 500.0) * (rng() % 5 ? 1.f : -1.f);
        t.offset[i] = (float)((double)(rng() % 1000) / 500.0 - 0.5);
    }
    return t;
}

struct Leaf {
    double lo[3], hi[3];
};

// the dense leaves by a walk of its own (doubles are exact for these coordinates)
void walk(const Tree& t, int64_t n, int lvl, const double org[3], std::vector<Leaf>& out) {
    const double size = std::ldexp(1.0, -(lvl + 1));
    for (int s = 0; s < 8; ++s) {
        const double o[3] = {org[0] + ((s >> 2) & 1) * size, org[1] + ((s >> 1) & 1) * size, org[2] + (s & 1) * size};
        const int32_t c = t.child[(size_t)n * 8 + s];
        if (c) {
            walk(t, n + c, lvl + 1, o, out);
        } else if (rto::half_to_float(t.sigma[((size_t)n * 8 + s) * t.stride]) > 0.f) {
            out.push_back({{o[0], o[1], o[2]}, {o[0] + size, o[1] + size, o[2] + size}});
        }
    }
}

// record r of `v` in tree units, margin taken off: lo / hi per axis
void tree_box(const Tree& t, const std::vector<float>& v, size_t r, double lo[3], double hi[3]) {
    for (int i = 0; i < 3; ++i) {
        const double c = (double)v[r * 8 + i] * t.scale[i] + t.offset[i], h = (double)v[r * 8 + 4 + i] - kMargin;
        lo[i] = c - h, hi[i] = c + h;
    }
}

bool fail(const char* what, int it) {
    std::fprintf(stderr, "tree %d: %s\n", it, what);
    return false;
}

// what holds for every child[] that culling_cells accepts
bool check_records(const Tree& t, const std::vector<float>& cells, const std::vector<float>& cubes, int it) {
    if (cells.size() != cubes.size() || cells.size() % 8) return fail("cells and cubes differ in size, or hold part of a record", it);
    for (size_t r = 0; r < cells.size() / 8; ++r) {
        if (cubes[r * 8 + 4] != cubes[r * 8 + 5] || cubes[r * 8 + 4] != cubes[r * 8 + 6]) return fail("a cube with unequal half-extents", it);
        if (cells[r * 8 + 3] != 0.f || cells[r * 8 + 7] != 0.f || cubes[r * 8 + 3] != 0.f || cubes[r * 8 + 7] != 0.f)
            return fail("a record's spare floats are not 0", it);
        if ((double)cubes[r * 8 + 4] - kMargin < std::ldexp(0.5, -rto::kOccLevel) - 1e-9) return fail("a cube finer than the culling level", it);
        double bl[3], bh[3], cl[3], ch[3];
        tree_box(t, cells, r, bl, bh);
        tree_box(t, cubes, r, cl, ch);
        for (int i = 0; i < 3; ++i) {
            const double tol = kTol * (1.0 + std::fabs(t.offset[i]) + std::fabs(bl[i]) + std::fabs(bh[i]));
            if (!(bl[i] < bh[i])) return fail("empty or NaN bounds", it);
            if (bl[i] < cl[i] - tol || bh[i] > ch[i] + tol) return fail("bounds outside their cell", it);
        }
    }
    return true;
}

bool check_tree(const Tree& t, int it) {
    std::vector<float> cells, cubes, alone;
    if (!rto::culling_cells(t.child.data(), t.capacity, t.scale, t.offset, t.sigma.data(), t.stride, cells, &cubes))
        return fail("a breadth-first tree was refused", it);
    if (!rto::culling_cells(t.child.data(), t.capacity, t.scale, t.offset, t.sigma.data(), t.stride, alone) || alone != cells)
        return fail("the cells depend on whether the cubes are asked for", it);
    if (!check_records(t, cells, cubes, it)) return false;
    std::vector<Leaf> leaves;
    const double org[3] = {0, 0, 0};
    walk(t, 0, 0, org, leaves);
    if (leaves.empty() != cells.empty()) return fail("cells without a dense leaf, or dense leaves without a cell", it);
    const size_t nr = cells.size() / 8;
    std::vector<int> faces(nr, 0);  // bit 2 i: a leaf face on the low face of axis i, bit 2 i + 1: on the high one
    // the cube of level lv that holds point p, as a key; the cubes are disjoint, so a leaf's centre names its cell
    auto key = [](int lv, const double p[3]) {
        uint64_t k = (uint64_t)lv;
        for (int i = 0; i < 3; ++i) k = k << 16 | (uint64_t)std::floor(std::ldexp(p[i], lv));
        return k;
    };
    std::map<uint64_t, size_t> by_cube;
    for (size_t r = 0; r < nr; ++r) {
        double cl[3], ch[3];
        tree_box(t, cubes, r, cl, ch);
        const double mid[3] = {0.5 * (cl[0] + ch[0]), 0.5 * (cl[1] + ch[1]), 0.5 * (cl[2] + ch[2])};
        if (!by_cube.emplace(key((int)std::lround(-std::log2(ch[0] - cl[0])), mid), r).second) return fail("two cells with one cube", it);
    }
    for (const Leaf& l : leaves) {
        size_t owner = nr;
        const double mid[3] = {0.5 * (l.lo[0] + l.hi[0]), 0.5 * (l.lo[1] + l.hi[1]), 0.5 * (l.lo[2] + l.hi[2])};
        for (int lv = 1; lv <= rto::kOccLevel && owner == nr; ++lv) {
            const auto f = by_cube.find(key(lv, mid));
            if (f != by_cube.end()) owner = f->second;
        }
        if (owner == nr) return fail("a dense leaf in no cell's cube", it);
        double bl[3], bh[3];
        tree_box(t, cells, owner, bl, bh);
        for (int i = 0; i < 3; ++i) {
            const double tol = kTol * (1.0 + std::fabs(t.offset[i]) + std::fabs(bl[i]) + std::fabs(bh[i]));
            if (l.lo[i] < bl[i] - tol || l.hi[i] > bh[i] + tol) return fail("a dense leaf sticks out of its cell's bounds", it);
            if (std::fabs(l.lo[i] - bl[i]) <= tol) faces[owner] |= 1 << (2 * i);
            if (std::fabs(l.hi[i] - bh[i]) <= tol) faces[owner] |= 2 << (2 * i);
        }
    }
    for (size_t r = 0; r < nr; ++r)
        if (faces[r] != 63) return fail("bounds wider than the dense leaves of their cell", it);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937_64 rng(argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1);
    size_t n_cells = 0, tight = 0, accepted = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        Tree t = random_tree(rng);
        if (!check_tree(t, it)) return 1;
        std::vector<float> cells, cubes;
        rto::culling_cells(t.child.data(), t.capacity, t.scale, t.offset, t.sigma.data(), t.stride, cells, &cubes);
        n_cells += cells.size() / 8;
        for (size_t r = 0; r < cells.size() / 8; ++r) tight += cells[r * 8 + 4] < cubes[r * 8 + 4] || cells[r * 8 + 5] < cubes[r * 8 + 5] || cells[r * 8 + 6] < cubes[r * 8 + 6];
        for (int m = 0; m < 8; ++m) {  // damaged child arrays: offsets anywhere, reachable nodes included
            Tree d = t;
            for (int k = 0, nk = 1 + (int)(rng() % 6); k < nk; ++k) {
                int32_t& c = d.child[(size_t)(rng() % d.child.size())];
                switch (rng() % 5) {
                    case 0: c = (int32_t)(rng() % (uint64_t)(d.capacity + 2)); break;         // forward: a second parent, or just past the end
                    case 1: c = -(int32_t)(rng() % (uint64_t)(d.capacity + 2)); break;        // backwards
                    case 2: c = (int32_t)rng(); break;                                        // anything
                    case 3: c = c ? 0 : 1; break;                                             // a leaf <-> the next node
                    default: c = rng() % 2 ? INT32_MAX : INT32_MIN; break;
                }
            }
            if (rto::culling_cells(d.child.data(), d.capacity, d.scale, d.offset, d.sigma.data(), d.stride, cells, &cubes)) {
                ++accepted;
                if (!check_records(d, cells, cubes, it)) return 1;
            } else {
                ++refused;
            }
        }
    }
    std::printf("culling_cells: %d trees, %zu cells (%zu with bounds tighter than the cube); %zu damaged child arrays accepted, %zu refused: "
                "clean under ASan + UBSan\n", iters, n_cells, tight, accepted, refused);
    return tight && accepted && refused ? 0 : 1;  // (a run that never met a case proves nothing about it)
}
