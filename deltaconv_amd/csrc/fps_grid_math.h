// The rules of exact Euclidean farthest-point sampling over a uniform cell grid (fps_grid.hip: dc_fps_grid), shared with the g++
// host-check build (tests/hostcheck_fps_grid) like fps_euclid_math.h / knn_grid_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// EXACT: the picks of dcfpse::sample (fps_euclid_math.h) bit for bit.  State (one fp32 key md per point: +inf, NONFINITE, PICKED),
// update, the 64-bit selection key (image(md), ~id), clamp_start and "a pick index r >= n gets -1" are that header's, unchanged.
// The grid only decides WHICH points a pick looks at; it is dcgrid::make_grid over the cloud's finite points with cell_axis /
// cell_of (knn_grid_math.h), so the same grid build serves both.  A point with a non-finite coordinate belongs to no cell.
//
// The box of a pick.  When the picked point c is finite and at least one more pick follows, let D be the md c held when it was
// selected (+inf for the start, and for the pick after a non-finite start: every finite point still holds +inf then).
//   R    = the smallest r in 0 .. rcover with dcgrid::bound2(r, min_h) >= D, or rcover where there is none; rcover = the Chebyshev
//          radius around c's cell that covers the grid (cover_radius)
//   box  = the cells at Chebyshev distance <= R from c's cell, clipped to the grid
//   every finite point of a box cell gets dcfpse::update against c; c itself becomes PICKED; no other point is read
//   a non-finite pick updates nothing, and the last pick of a cloud updates nothing
//   stats[0] += the number of points in the box's cells (picked ones included), stats[1] += the number of cells of the box:
//   functions of the inputs and the target alone, whatever walks the box
//
// Proof that the points outside the box keep their md, so that the state after every pick is dcfpse::sample's.
//   1. D is the maximum.  c was selected as the maximum key, so md(p) <= D for every unpicked finite p; a picked point holds
//      PICKED < 0 and update() leaves it alone (md >= 0 is false).  D >= 0: it is +inf or a rounded sum of squares.
//   2. Outside the box d2 >= bound2(R).  For R >= 1 the claim of knn_grid_math.h reads: a point p in a cell at Chebyshev distance
//      > R from the cell of c has COMPUTED dcgrid::dist2(c, p) >= bound2(R, min_h).  update() computes dcinterp::dist2(p, c);
//      the two are the same value: fl(a - b) = -fl(b - a) per axis, the squares are equal, and the sums add the same three
//      numbers in the same order.  (c is a point of the cloud, hence inside the bounding box: the claim's plain case.)
//   3. Hence for p outside the box: d2 >= bound2(R) >= D >= md(p), so `d2 < md` is false and update() returns md(p): skipping p
//      changes nothing.  A NaN d2 (overflow to inf - inf cannot occur between finite points; inf d2 can) lowers nothing either way.
//   4. R = 0 is chosen only where bound2(0) = 0 >= D, that is D = 0.  Then every unpicked finite point holds md <= 0, so md = 0
//      (or it is picked), and `d2 < 0` is false for every point: nothing outside c's own cell could change -- because D = 0, not
//      because of the claim, which says nothing for r = 0.  The points of c's own cell are visited anyway (c must be marked).
//   5. D above B2_MAX (+inf included): bound2 is cut to B2_MAX < D for every r, no r qualifies, the box is the whole grid: brute
//      force.  bound2 = 0 below B2_MIN (cells so small that the bound underflows, or a one-cell grid with min_h = 0): no r
//      qualifies unless D = 0, the box is the whole grid: no pruning, still correct.
//   6. The whole grid (R = rcover) leaves no point outside, so nothing is to prove there.
//
// Selection.  One key per cell, the maximum of dcfpse::key(md, id) over its points (0 for an empty cell), and one key per block of
// BLOCK_CELLS consecutive cells; the maximum over the blocks is the maximum over all finite points, and only the cells of the box
// (and the blocks that hold one) can have changed.  A key with its top bit set belongs to a finite unpicked point (md >= 0).
// Non-finite tail: when the maximum key has its top bit clear (PICKED, or 0: no finite point at all), every finite point is taken.
// The remaining picks are the rows with a non-finite coordinate in ascending id, without the start if it was one of them -- what
// dcfpse::sample does with their common NONFINITE key.
#pragma once
#include <stdint.h>

#include "fps_euclid_math.h"
#include "knn_grid_math.h"

namespace dcfpsg {

constexpr int MAX_POINTS = 262144;            // DC_FPS_GRID_MAX_POINTS: 2 n cells -> n / 32 block keys of 8 bytes in LDS (64 KiB)
constexpr int BLOCK_CELLS = 64;               // cells of a block key: one wave reads a block
constexpr float DEFAULT_TARGET = 0.5f;        // mean points per cell where the caller names none (README: the best measured)

typedef unsigned long long u64;

DC_HD bool key_live(u64 k) { return (k >> 63) != 0; }                  // image(md) of an md >= 0: a finite, unpicked point
// the md inside a key (the inverse of dcfpse::image)
DC_HD float key_md(u64 k) {
    const uint32_t im = (uint32_t)(k >> 32);
    union { uint32_t u; float f; } c;
    c.u = (im & 0x80000000u) ? (im & 0x7fffffffu) : ~im;
    return c.f;
}
DC_HD int blocks_of(int cells) { return (cells + BLOCK_CELLS - 1) / BLOCK_CELLS; }

// the Chebyshev radius around cell (cx, cy, cz) that covers the grid
DC_HD int cover_radius(const dcgrid::Grid& G, int cx, int cy, int cz) {
    int r = cx > G.g[0] - 1 - cx ? cx : G.g[0] - 1 - cx;
    r = cy > r ? cy : r;
    r = G.g[1] - 1 - cy > r ? G.g[1] - 1 - cy : r;
    r = cz > r ? cz : r;
    r = G.g[2] - 1 - cz > r ? G.g[2] - 1 - cz : r;
    return r;
}
// the smallest r in 0 .. rcover with bound2(r) >= D, or rcover (bound2 is non-decreasing in r: rounded products of non-negatives)
DC_HD int box_radius(float D, float min_h, int rcover) {
    int r = 0;
    while (r < rcover && !(dcgrid::bound2(r, min_h) >= D)) ++r;
    return r;
}

// The box of a pick, clipped to the grid, as runs of consecutive cell ids (cell id = (z g1 + y) g0 + x: a run along x; whole
// rows of one z join into one run, whole slabs into one).
struct Box {
    int x0, y0, z0, nx, ny, nz;               // first cell and cells per axis
    int runs, run_cells;                      // `runs` runs of `run_cells` cells each
    int kind;                                 // 0: one run along x per (y, z); 1: one run per z (whole rows); 2: one run (whole slabs)
};
DC_HD Box make_box(const dcgrid::Grid& G, int cx, int cy, int cz, int R) {
    Box b;
    b.x0 = cx - R > 0 ? cx - R : 0;
    b.y0 = cy - R > 0 ? cy - R : 0;
    b.z0 = cz - R > 0 ? cz - R : 0;
    b.nx = (cx + R < G.g[0] - 1 ? cx + R : G.g[0] - 1) - b.x0 + 1;
    b.ny = (cy + R < G.g[1] - 1 ? cy + R : G.g[1] - 1) - b.y0 + 1;
    b.nz = (cz + R < G.g[2] - 1 ? cz + R : G.g[2] - 1) - b.z0 + 1;
    if (b.nx == G.g[0] && b.ny == G.g[1]) {
        b.kind = 2;
        b.runs = 1;
        b.run_cells = b.nx * b.ny * b.nz;
    } else if (b.nx == G.g[0]) {
        b.kind = 1;
        b.runs = b.nz;
        b.run_cells = b.nx * b.ny;
    } else {
        b.kind = 0;
        b.runs = b.ny * b.nz;
        b.run_cells = b.nx;
    }
    return b;
}
DC_HD long long box_cells(const Box& b) { return (long long)b.nx * b.ny * b.nz; }
// first cell of run i
DC_HD int run_first(const dcgrid::Grid& G, const Box& b, int i) {
    if (b.kind == 2) return dcgrid::cell_of(G, 0, 0, b.z0);
    if (b.kind == 1) return dcgrid::cell_of(G, 0, b.y0, b.z0 + i);
    return dcgrid::cell_of(G, b.x0, b.y0 + i % b.ny, b.z0 + i / b.ny);
}
// cell i of the box, i in [0, box_cells)
DC_HD int box_cell(const dcgrid::Grid& G, const Box& b, long long i) {
    const int x = (int)(i % b.nx), y = (int)((i / b.nx) % b.ny), z = (int)(i / ((long long)b.nx * b.ny));
    return dcgrid::cell_of(G, b.x0 + x, b.y0 + y, b.z0 + z);
}

}  // namespace dcfpsg

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace dcfpsg {

// The whole sample of one cloud as plain loops: pos [n,3] -> picks [m] local ids in pick order (-1 for a pick index r >= n),
// stats [2] (may be null).  The same grid, cell-ordered points, cell and block keys and box walk as the kernel, one after another.
inline void sample(const float* pos, int n, int m, int start, float target, int32_t* picks, int64_t* stats) {
    using dcgrid::Grid;
    using dcgrid::Pt;
    int64_t st[2] = {0, 0};
    float lo[3] = {dcgrid::inf(), dcgrid::inf(), dcgrid::inf()}, hi[3] = {-dcgrid::inf(), -dcgrid::inf(), -dcgrid::inf()};
    long long fin = 0;
    for (int i = 0; i < n; ++i) {
        const float* p = pos + 3 * i;
        if (!dcgrid::finite3(p[0], p[1], p[2])) continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = p[a] < lo[a] ? p[a] : lo[a];
            hi[a] = p[a] > hi[a] ? p[a] : hi[a];
        }
        ++fin;
    }
    Grid G;
    dcgrid::make_grid(fin, lo, hi, target, G);
    auto cell_at = [&](const float* p) {
        return dcgrid::cell_of(G, dcgrid::cell_axis(p[0], G.lo[0], G.inv_h[0], G.g[0]), dcgrid::cell_axis(p[1], G.lo[1], G.inv_h[1], G.g[1]),
                               dcgrid::cell_axis(p[2], G.lo[2], G.inv_h[2], G.g[2]));
    };
    std::vector<long long> cstart((size_t)G.cells + 1, 0), cursor((size_t)G.cells, 0);
    for (int i = 0; i < n; ++i)
        if (dcgrid::finite3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])) ++cstart[(size_t)cell_at(pos + 3 * i) + 1];
    for (int c = 0; c < G.cells; ++c) cstart[c + 1] += cstart[c];
    std::vector<Pt> pts((size_t)fin);
    for (int i = 0; i < n; ++i) {
        const float* p = pos + 3 * i;
        if (!dcgrid::finite3(p[0], p[1], p[2])) continue;
        const int c = cell_at(p);
        pts[(size_t)(cstart[c] + cursor[c]++)] = Pt{p[0], p[1], p[2], i};
    }
    std::vector<float> md((size_t)fin, dcfpse::inf());
    const int nblk = blocks_of(G.cells);
    std::vector<u64> ckey((size_t)G.cells, 0ull), bkey((size_t)nblk, 0ull);
    auto cell_key = [&](int c) {
        u64 k = 0ull;
        for (long long j = cstart[c]; j < cstart[c + 1]; ++j) {
            const u64 kj = dcfpse::key(md[(size_t)j], pts[(size_t)j].id);
            k = kj > k ? kj : k;
        }
        ckey[c] = k;
    };
    auto block_key = [&](int b) {
        u64 k = 0ull;
        for (int c = b * BLOCK_CELLS; c < (b + 1) * BLOCK_CELLS && c < G.cells; ++c) k = ckey[c] > k ? ckey[c] : k;
        bkey[b] = k;
    };
    for (int c = 0; c < G.cells; ++c) cell_key(c);
    for (int b = 0; b < nblk; ++b) block_key(b);

    const int count = m < n ? m : n;
    int cur = n > 0 ? dcfpse::clamp_start(start, n) : 0, r = 0;
    float D = dcfpse::inf();
    bool tail = false;
    for (; r < count; ++r) {
        picks[r] = cur;
        if (r + 1 == count) {
            ++r;
            break;
        }
        const float cx = pos[3 * cur], cy = pos[3 * cur + 1], cz = pos[3 * cur + 2];
        if (dcgrid::finite3(cx, cy, cz)) {
            const int ix = dcgrid::cell_axis(cx, G.lo[0], G.inv_h[0], G.g[0]), iy = dcgrid::cell_axis(cy, G.lo[1], G.inv_h[1], G.g[1]),
                      iz = dcgrid::cell_axis(cz, G.lo[2], G.inv_h[2], G.g[2]);
            const int R = box_radius(D, G.min_h, cover_radius(G, ix, iy, iz));
            const Box box = make_box(G, ix, iy, iz, R);
            for (int i = 0; i < box.runs; ++i) {
                const int c0 = run_first(G, box, i);
                for (long long j = cstart[c0]; j < cstart[c0 + box.run_cells]; ++j) {
                    const Pt& p = pts[(size_t)j];
                    md[(size_t)j] = dcfpse::update(md[(size_t)j], p.id == cur, p.x, p.y, p.z, cx, cy, cz);
                }
                st[0] += cstart[c0 + box.run_cells] - cstart[c0];
            }
            st[1] += box_cells(box);
            for (long long i = 0; i < box_cells(box); ++i) cell_key(box_cell(G, box, i));
            for (int i = 0; i < box.runs; ++i) {
                const int c0 = run_first(G, box, i);
                for (int b = c0 / BLOCK_CELLS; b <= (c0 + box.run_cells - 1) / BLOCK_CELLS; ++b) block_key(b);
            }
        }
        u64 best = 0ull;
        for (int b = 0; b < nblk; ++b) best = bkey[b] > best ? bkey[b] : best;
        if (!key_live(best)) {
            ++r;
            tail = true;
            break;
        }
        cur = dcfpse::key_id(best);
        D = key_md(best);
    }
    if (tail) {                               // the rows with a non-finite coordinate, ascending, without the start
        const int s = dcfpse::clamp_start(start, n);
        for (int i = 0; i < n && r < count; ++i)
            if (i != s && !dcgrid::finite3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])) picks[r++] = i;
    }
    for (r = count; r < m; ++r) picks[r] = -1;
    if (stats) {
        stats[0] = st[0];
        stats[1] = st[1];
    }
}

}  // namespace dcfpsg
#endif
