// g++ build of deltaconv_amd/csrc/fps_grid_math.h -- the rules of dc_fps_grid (fps_grid.hip): the box of a pick, the cell and block
// keys, the non-finite tail -- with the sample of one cloud as plain loops on the CPU, beside dcfpse::sample, the brute-force
// oracle (tests/test_fps_grid_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/fps_grid_math.h"

extern "C" {

int32_t hg_max_points(void) { return dcfpsg::MAX_POINTS; }
int32_t hg_block_cells(void) { return dcfpsg::BLOCK_CELLS; }
float hg_default_target(void) { return dcfpsg::DEFAULT_TARGET; }

// one cloud: pos [n,3] -> picks [m] local ids in pick order (-1 for a pick index at or above n), stats [2].  -> 0, or -1 for bad sizes
int hg_sample(const float* pos, int64_t n, int32_t m, int32_t start, float target, int32_t* picks, int64_t* stats) {
    if (n < 0 || m < 0 || n > 0x7fffffff || (n > 0 && !pos) || (m > 0 && !picks) || !(target > 0.f) || !dcgrid::finite1(target)) return -1;
    dcfpsg::sample(pos, (int)n, m, start, target, picks, stats);
    return 0;
}

// the same cloud by brute force (fps_euclid_math.h)
int hg_sample_brute(const float* pos, int64_t n, int32_t m, int32_t start, int32_t* picks) {
    if (n < 0 || m < 0 || n > 0x7fffffff || (n > 0 && !pos) || (m > 0 && !picks)) return -1;
    std::vector<float> md((size_t)n);
    dcfpse::sample(pos, (int)n, m, start, md.data(), picks);
    return 0;
}

// key_md(key(md, id)) -> out [n]: the inverse image
void hg_key_md(const float* md, const int32_t* id, int64_t n, float* out, int32_t* live) {
    for (int64_t i = 0; i < n; ++i) {
        const unsigned long long k = dcfpse::key(md[i], id[i]);
        out[i] = dcfpsg::key_md(k);
        live[i] = dcfpsg::key_live(k) ? 1 : 0;
    }
}

}  // extern "C"
