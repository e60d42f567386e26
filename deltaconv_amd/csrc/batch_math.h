// Per-draw and per-point arithmetic of the batch assembly kernel (batch.hip), shared with the g++ host-check build
// (tests/hostcheck_batch) like point_math.h / nn_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated: the training-time augmentations of /root/reference/experiments/train_*.py --
//   scale          deltaconv/transforms/random_scale.py:24-35   three factors per cloud; pos *= s; norm *= 1/s, re-normalised
//   rotate         deltaconv/transforms/random_rotate.py:28-45  one angle per cloud; pos @ R, norm @ R
//   translate      deltaconv/transforms/random_translate_global.py:23-36  one offset per cloud and axis in (-t, t)
//   normal jitter  deltaconv/transforms/random_normals.py:25-36 per point and axis, then norm / max(|norm|, 1e-5)
//   point jitter   torch_geometric.transforms.RandomTranslate (train_scanobjectnn.py:49): per point and axis, added to pos
//
// Draws: Philox-4x32-10 (nn_math.h), key = (seed, BATCH_KEY), counter =
//     x = point index inside its cloud, or PER_CLOUD (0xFFFFFFFF) for a per-cloud draw
//     y = index of the cloud in the DATASET (not its slot in the batch)
//     z = low 32 bits of `step`
//     w = (bits 32..60 of `step`) << 3 | position of the op in the op list (0..7)
// so every (seed, step, cloud, op position, point | per-cloud) has a counter of its own (0 <= step < 2^61; a cloud has fewer
// than 2^32 - 1 points).  Words x, y, z of the output serve axes 0, 1, 2 (the angle of a rotation: word x).
// A uniform draw is u = (r >> 8) * 2^-24 in [0, 1), value = lo + u * (hi - lo): fp32, every operation rounded on its own
// (the library is built with -ffp-contract=off), so a numpy float32 restatement reproduces every drawn parameter bit for bit.
#pragma once
#include "nn_math.h"

namespace dcbatch {

enum { OP_SCALE = 1, OP_ROTATE = 2, OP_TRANSLATE = 3, OP_NORMAL_JITTER = 4, OP_POINT_JITTER = 5 };
constexpr int MAX_OPS = 8;
constexpr unsigned BATCH_KEY = 0x6261746Bu;   // "batk"; the dropout's streams use 0x64726F70
constexpr unsigned PER_CLOUD = 0xFFFFFFFFu;
constexpr float NORMAL_EPS = 1e-5f;           // random_normals.py:34

DC_HD dcnn::U4 draw(unsigned seed, long long step, unsigned cloud, int op_pos, unsigned point) {
    const unsigned long long s = (unsigned long long)step;
    return dcnn::philox4x32_10(dcnn::U4{point, cloud, (unsigned)s, ((unsigned)(s >> 32) << 3) | (unsigned)op_pos}, seed, BATCH_KEY);
}
DC_HD float uniform(unsigned r, float lo, float hi) {
    const float u = (float)(r >> 8) * (1.0f / 16777216.0f);
    const float w = hi - lo;
    const float t = u * w;
    return lo + t;
}

// What an op needs per CLOUD, three floats:
//   scale      (sx, sy, sz)                     from params (lo, hi, -)
//   rotate     (sin a, cos a, degrees drawn)    from params (deg_lo, deg_hi, axis); a = degrees * (pi / 180) in fp32
//   translate  (ox, oy, oz)                     from params (tx, ty, tz): uniform in (-|t|, |t|)
//   jitters    nothing (their draws are per point)
DC_HD void cloud_draw(int code, const float* prm, unsigned seed, long long step, unsigned cloud, int op_pos, float* out) {
    out[0] = out[1] = out[2] = 0.f;
    if (code != OP_SCALE && code != OP_ROTATE && code != OP_TRANSLATE) return;
    const dcnn::U4 r = draw(seed, step, cloud, op_pos, PER_CLOUD);
    if (code == OP_SCALE) {
        out[0] = uniform(r.x, prm[0], prm[1]);
        out[1] = uniform(r.y, prm[0], prm[1]);
        out[2] = uniform(r.z, prm[0], prm[1]);
    } else if (code == OP_ROTATE) {
        const float deg = uniform(r.x, prm[0], prm[1]);
        const float a = deg * 0.017453292519943295f;
        float sn, cs;
        sincosf(a, &sn, &cs);
        out[0] = sn;
        out[1] = cs;
        out[2] = deg;
    } else {
        out[0] = uniform(r.x, -fabsf(prm[0]), fabsf(prm[0]));
        out[1] = uniform(r.y, -fabsf(prm[1]), fabsf(prm[1]));
        out[2] = uniform(r.z, -fabsf(prm[2]), fabsf(prm[2]));
    }
}

// the three per-point offsets of a jitter op (params tx, ty, tz)
DC_HD void point_draw(const float* prm, unsigned seed, long long step, unsigned cloud, int op_pos, unsigned point, float* out) {
    const dcnn::U4 r = draw(seed, step, cloud, op_pos, point);
    out[0] = uniform(r.x, -fabsf(prm[0]), fabsf(prm[0]));
    out[1] = uniform(r.y, -fabsf(prm[1]), fabsf(prm[1]));
    out[2] = uniform(r.z, -fabsf(prm[2]), fabsf(prm[2]));
}

// v @ R for the matrices of random_rotate.py:35-40
DC_HD void rotate(int axis, float sn, float cs, float& x, float& y, float& z) {
    if (axis == 0) {            // [[1, 0, 0], [0, c, s], [0, -s, c]]
        const float a = y * cs - z * sn, b = y * sn + z * cs;
        y = a; z = b;
    } else if (axis == 1) {     // [[c, 0, -s], [0, 1, 0], [s, 0, c]]
        const float a = x * cs + z * sn, b = z * cs - x * sn;
        x = a; z = b;
    } else {                    // [[c, s, 0], [-s, c, 0], [0, 0, 1]]
        const float a = x * cs - y * sn, b = x * sn + y * cs;
        x = a; y = b;
    }
}

// One op on one point.  cw: the op's per-cloud values (cloud_draw); prm: its three parameters.  has_norm = 0: the normal
// part of scale / rotate is skipped, as the CPU classes do on a shape without normals.
DC_HD void apply_op(int code, const float* prm, const float* cw, unsigned seed, long long step, unsigned cloud, int op_pos,
                    unsigned point, int has_norm, float& px, float& py, float& pz, float& nx, float& ny, float& nz) {
    if (code == OP_SCALE) {
        px *= cw[0]; py *= cw[1]; pz *= cw[2];
        if (has_norm) {
            nx *= 1.f / cw[0]; ny *= 1.f / cw[1]; nz *= 1.f / cw[2];
            const float len = sqrtf(nx * nx + ny * ny + nz * nz);
            nx /= len; ny /= len; nz /= len;
        }
    } else if (code == OP_ROTATE) {
        const int axis = (int)prm[2];
        rotate(axis, cw[0], cw[1], px, py, pz);
        if (has_norm) rotate(axis, cw[0], cw[1], nx, ny, nz);
    } else if (code == OP_TRANSLATE) {
        px += cw[0]; py += cw[1]; pz += cw[2];
    } else if (code == OP_NORMAL_JITTER) {
        float j[3];
        point_draw(prm, seed, step, cloud, op_pos, point, j);
        nx += j[0]; ny += j[1]; nz += j[2];
        const float len = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), NORMAL_EPS);
        nx /= len; ny /= len; nz /= len;
    } else if (code == OP_POINT_JITTER) {
        float j[3];
        point_draw(prm, seed, step, cloud, op_pos, point, j);
        px += j[0]; py += j[1]; pz += j[2];
    }
}

}  // namespace dcbatch
