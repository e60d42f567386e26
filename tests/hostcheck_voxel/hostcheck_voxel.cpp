// g++ build of deltaconv_amd/csrc/voxel_math.h -- the rules of dc_voxel_subsample (voxel.hip): which points take part, the cell,
// the range, the key a point bids for its cell with -- with the subsampling of a batch as plain serial loops on the CPU: an ordered
// map per cloud instead of the device's hash table, a running count instead of its scan (tests/test_voxel_host.py).
#include <stdint.h>

#include <map>
#include <vector>

#include "../../deltaconv_amd/csrc/voxel_math.h"

extern "C" {

int32_t hv_axis_limit(void) { return (int32_t)dcvox::AXIS_LIMIT; }

// the key of (d2, index) pairs -> out [n] (the order the device's unsigned minimum sees)
void hv_keys(const float* d2, const uint32_t* id, int64_t n, uint64_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = dcvox::rep_key(d2[i], id[i]);
}

// one cloud's points against one origin: cell [n] (all ones: none) and key [n] of every point, flags [n]: 1 finite, 2 overflow
void hv_bids(const float* pos, int64_t n, const float* origin, const float* size, int32_t pick, uint64_t* cell, uint64_t* key,
             int32_t* flags) {
    for (int64_t i = 0; i < n; ++i) {
        const dcvox::Bid b = dcvox::bid(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], origin, size, pick, (uint32_t)i);
        cell[i] = b.cell;
        key[i] = b.key;
        flags[i] = (b.finite ? 1 : 0) | (b.overflow ? 2 : 0);
    }
}

// A batch: pos [N,3], ptr [B+1] row offsets, size [3], origin [B,3] or null (every cloud's own fp32 minimum over its finite points),
// pick -> rows [N] (the first optr[B] are written), optr [B+1], cluster [N].  Returns the first overflowing cloud, -1 for none,
// -2 for bad arguments.
int64_t hv_subsample(const float* pos, const int64_t* ptr, int32_t B, const float* size, const float* origin, int32_t pick,
                     int64_t* rows, int64_t* optr, int64_t* cluster) {
    if (B < 0 || !ptr || !size || !optr) return -2;
    int64_t over = -1, out = 0;
    optr[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t base = ptr[b], n = ptr[b + 1] - base;
        if (n < 0) return -2;
        float o[3] = {0.f, 0.f, 0.f};
        if (origin) {
            for (int a = 0; a < 3; ++a) o[a] = origin[3 * b + a];
        } else {
            float lo[3] = {dcgrid::inf(), dcgrid::inf(), dcgrid::inf()};
            for (int64_t i = 0; i < n; ++i) {
                const float* p = pos + 3 * (base + i);
                if (!dcgrid::finite3(p[0], p[1], p[2])) continue;
                for (int a = 0; a < 3; ++a) lo[a] = p[a] < lo[a] ? p[a] : lo[a];
            }
            for (int a = 0; a < 3; ++a) o[a] = lo[a] < dcgrid::inf() ? lo[a] : 0.f;
        }
        std::map<uint64_t, uint64_t> best;                   // cell -> smallest key
        std::vector<uint64_t> cell((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const float* p = pos + 3 * (base + i);
            const dcvox::Bid bid = dcvox::bid(p[0], p[1], p[2], o, size, pick, (uint32_t)i);
            cell[(size_t)i] = bid.cell;
            if (bid.overflow && over < 0) over = b;
            if (!bid.finite || bid.overflow) continue;
            auto it = best.find(bid.cell);
            if (it == best.end()) best[bid.cell] = bid.key;
            else if (bid.key < it->second) it->second = bid.key;
        }
        std::vector<int64_t> rank((size_t)n, -1);             // of a representative, by its local row
        for (int64_t i = 0; i < n; ++i) {
            if (cell[(size_t)i] == dcvox::EMPTY) continue;
            if ((int64_t)(best[cell[(size_t)i]] & 0xffffffffull) == i) {
                rows[out] = base + i;
                rank[(size_t)i] = out++;
            }
        }
        for (int64_t i = 0; i < n; ++i)
            cluster[base + i] = cell[(size_t)i] == dcvox::EMPTY ? -1 : rank[(size_t)(best[cell[(size_t)i]] & 0xffffffffull)];
        optr[b + 1] = out;
    }
    return over;
}

}  // extern "C"
