// g++ build of deltaconv_amd/csrc/batch_math.h -- the draws and the per-point ops of the batch assembly kernel (batch.hip),
// looped over clouds / points on the CPU (tests/test_loader_host.py).
#include <stdint.h>

#include "../../deltaconv_amd/csrc/batch_math.h"

extern "C" {

// out [n_clouds, n_ops, 3]: what the kernel keeps per cloud and op (scale factors | sin, cos, degrees | offsets | zeros)
void hb_cloud_draws(const int32_t* codes, const float* prm, int n_ops, uint32_t seed, int64_t step, const int64_t* clouds,
                    int n_clouds, float* out) {
    for (int c = 0; c < n_clouds; ++c)
        for (int o = 0; o < n_ops; ++o)
            dcbatch::cloud_draw(codes[o], prm + 3 * o, seed, step, (unsigned)clouds[c], o, out + ((long)c * n_ops + o) * 3);
}

// out [n, 3]: the per-point offsets of the jitter op at position op_pos
void hb_point_draws(const float* prm, uint32_t seed, int64_t step, int64_t cloud, int op_pos, int n, float* out) {
    for (int p = 0; p < n; ++p) dcbatch::point_draw(prm, seed, step, (unsigned)cloud, op_pos, (unsigned)p, out + 3L * p);
}

// the whole op list on the n points of one cloud; norm_in / norm_out may be null (a store without normals)
void hb_apply(const int32_t* codes, const float* prm, int n_ops, uint32_t seed, int64_t step, int64_t cloud, int n,
              const float* pos_in, const float* norm_in, float* pos_out, float* norm_out) {
    float cw[dcbatch::MAX_OPS * 3];
    for (int o = 0; o < n_ops; ++o) dcbatch::cloud_draw(codes[o], prm + 3 * o, seed, step, (unsigned)cloud, o, cw + 3 * o);
    for (int p = 0; p < n; ++p) {
        float px = pos_in[3L * p], py = pos_in[3L * p + 1], pz = pos_in[3L * p + 2], nx = 0.f, ny = 0.f, nz = 0.f;
        if (norm_in) { nx = norm_in[3L * p]; ny = norm_in[3L * p + 1]; nz = norm_in[3L * p + 2]; }
        for (int o = 0; o < n_ops; ++o)
            dcbatch::apply_op(codes[o], prm + 3 * o, cw + 3 * o, seed, step, (unsigned)cloud, o, (unsigned)p, norm_in != nullptr, px,
                              py, pz, nx, ny, nz);
        pos_out[3L * p] = px; pos_out[3L * p + 1] = py; pos_out[3L * p + 2] = pz;
        if (norm_in) { norm_out[3L * p] = nx; norm_out[3L * p + 1] = ny; norm_out[3L * p + 2] = nz; }
    }
}

}  // extern "C"
