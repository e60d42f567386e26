// g++ build of deltaconv_amd/csrc/fps_euclid_math.h -- the rules of dc_fps_batch (fps_euclid.hip): initial keys, the update after
// a pick, the 64-bit selection key -- with the sample of one cloud as plain loops on the CPU (tests/test_fps_euclid_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/fps_euclid_math.h"

extern "C" {

int32_t hf_max_points(void) { return dcfpse::MAX_POINTS; }

// one cloud: pos [n,3] -> picks [m] local ids in pick order (-1 for a pick index at or above n).  -> 0, or -1 for bad sizes
int hf_sample(const float* pos, int64_t n, int32_t m, int32_t start, int32_t* picks) {
    if (n < 0 || m < 0 || n > 0x7fffffff || (n > 0 && !pos) || (m > 0 && !picks)) return -1;
    std::vector<float> md((size_t)n);
    dcfpse::sample(pos, (int)n, m, start, md.data(), picks);
    return 0;
}

// the selection key of (md, id) pairs -> out [n] (the order the kernel's unsigned maximum sees)
void hf_keys(const float* md, const int32_t* id, int64_t n, uint64_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = dcfpse::key(md[i], id[i]);
}

}  // extern "C"
