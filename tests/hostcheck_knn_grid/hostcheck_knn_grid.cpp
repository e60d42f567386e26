// g++ build of deltaconv_amd/csrc/knn_grid_math.h -- the grid rule, the cell of a point, the stopping bound and the per-thread
// search of dc_knn_grid / dc_knn_cross_grid (knn_grid.hip), with the build (box, count, scan, fill) and the queries as plain loops
// on the CPU (tests/test_knn_grid_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/knn_grid_math.h"

namespace {

using dcgrid::Grid;
using dcgrid::Pt;

struct Built {
    Grid G;
    std::vector<Pt> pts;
    std::vector<int64_t> cstart;
};

// the build of one reference cloud: box over the finite points, make_grid, count, scan, fill (in index order inside a cell; `rev`
// fills in DESCENDING index order instead -- the device's order inside a cell is arbitrary and must not reach the result)
void build(const float* ref, int64_t nr, float target, int rev, Built& b) {
    float lo[3] = {dcgrid::inf(), dcgrid::inf(), dcgrid::inf()}, hi[3] = {-dcgrid::inf(), -dcgrid::inf(), -dcgrid::inf()};
    long long m = 0;
    for (int64_t i = 0; i < nr; ++i) {
        const float* p = ref + 3 * i;
        if (!dcgrid::finite3(p[0], p[1], p[2])) continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], p[a]);
            hi[a] = fmaxf(hi[a], p[a]);
        }
        ++m;
    }
    dcgrid::make_grid(m, lo, hi, target, b.G);
    const Grid& G = b.G;
    b.cstart.assign(G.cells + 1, 0);
    auto cell = [&](const float* p) {
        return dcgrid::cell_of(G, dcgrid::cell_axis(p[0], G.lo[0], G.inv_h[0], G.g[0]), dcgrid::cell_axis(p[1], G.lo[1], G.inv_h[1], G.g[1]),
                               dcgrid::cell_axis(p[2], G.lo[2], G.inv_h[2], G.g[2]));
    };
    for (int64_t i = 0; i < nr; ++i)
        if (dcgrid::finite3(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2])) ++b.cstart[cell(ref + 3 * i) + 1];
    for (int c = 0; c < G.cells; ++c) b.cstart[c + 1] += b.cstart[c];
    std::vector<int64_t> cursor(b.cstart.begin(), b.cstart.end() - 1);
    b.pts.resize(m);
    for (int64_t j = 0; j < nr; ++j) {
        const int64_t i = rev ? nr - 1 - j : j;
        const float* p = ref + 3 * i;
        if (dcgrid::finite3(p[0], p[1], p[2])) b.pts[cursor[cell(p)]++] = Pt{p[0], p[1], p[2], (int)i};
    }
}

// the queries of one cloud pair; self: idx gets the query's own id where nothing fills a slot, and no d2 is written
template <int K>
void run(const float* query, int64_t nq, const Built& b, int32_t k, int self, int32_t* idx, float* d2) {
    for (int64_t q = 0; q < nq; ++q) {
        const float* p = query + 3 * q;
        dcgrid::TopKLex<K> best;
        best.init();
        if (dcgrid::finite3(p[0], p[1], p[2]))
            dcgrid::search<K>(b.G, b.pts.data(), b.cstart.data(), (long long)b.pts.size(), p[0], p[1], p[2], k, best);
        for (int s = 0; s < k; ++s) {
            const bool empty = best.id[s] == 0x7fffffff;
            idx[q * k + s] = empty ? (self ? (int32_t)q : -1) : best.id[s];
            if (d2) d2[q * k + s] = best.d[s];
        }
    }
}

}  // namespace

extern "C" {

// -> out[12]: the Grid record as 32-bit words (lo 3, inv_h 3, g 3, min_h, m, cells)
void hg_make_grid(int64_t m, const float* lo, const float* hi, float target, uint32_t* out) {
    Grid G;
    dcgrid::make_grid(m, lo, hi, target, G);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&G);
    for (int i = 0; i < 12; ++i) out[i] = w[i];
}

// the grid of a cloud as the build sees it (box over its finite points) -> out[12]
void hg_grid_of(const float* ref, int64_t nr, float target, uint32_t* out) {
    Built b;
    build(ref, nr, target, 0, b);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&b.G);
    for (int i = 0; i < 12; ++i) out[i] = w[i];
}

// per-axis cells of n points under the grid record `grid` -> cells [n,3]
void hg_cells(const uint32_t* grid, const float* p, int64_t n, int32_t* cells) {
    const Grid& G = *reinterpret_cast<const Grid*>(grid);
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) cells[3 * i + a] = dcgrid::cell_axis(p[3 * i + a], G.lo[a], G.inv_h[a], G.g[a]);
}

void hg_bound2(const int32_t* r, int64_t n, float min_h, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = dcgrid::bound2(r[i], min_h);
}

// one cloud pair through the grid: query [nq,3], ref [nr,3] -> idx [nq,k], d2 [nq,k] (d2 may be null).  self = 1: the form of
// dc_knn_grid (K by its dispatch, k <= 64); self = 0: the form of dc_knn_cross_grid (k <= 16).  -> 0, or -1 for a k out of range
int hg_search(const float* query, int64_t nq, const float* ref, int64_t nr, int32_t k, float target, int32_t self, int32_t rev,
              int32_t* idx, float* d2) {
    if (k < 1 || k > (self ? 64 : 16)) return -1;
    Built b;
    build(ref, nr, target, rev, b);
    if (self) {
        if (k <= 10) run<10>(query, nq, b, k, 1, idx, d2);
        else if (k <= 16) run<16>(query, nq, b, k, 1, idx, d2);
        else if (k <= 20) run<20>(query, nq, b, k, 1, idx, d2);
        else if (k <= 30) run<30>(query, nq, b, k, 1, idx, d2);
        else if (k <= 40) run<40>(query, nq, b, k, 1, idx, d2);
        else run<64>(query, nq, b, k, 1, idx, d2);
    } else {
        if (k == 1) run<1>(query, nq, b, k, 0, idx, d2);
        else if (k <= 4) run<4>(query, nq, b, k, 0, idx, d2);
        else if (k <= 8) run<8>(query, nq, b, k, 0, idx, d2);
        else run<16>(query, nq, b, k, 0, idx, d2);
    }
    return 0;
}

}  // extern "C"
