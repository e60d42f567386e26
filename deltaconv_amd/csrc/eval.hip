// Evaluation metrics of a batch of logits in ONE launch: what the reference's test loops do on the host per batch
// (/root/reference/experiments/utils.py:27-51 calc_shape_IoU, test_shapenet.py:84-103: logits and labels copied to the host,
// np.argmax, a Python loop over shapes and parts) -- the optional vote accumulation `votes += logits`, the row arg-max, per-cloud
// per-class counts and the mean part IoU per shape.  One workgroup per cloud (rows ptr[b] .. ptr[b+1]); classification is the
// same entry with the batch as one cloud.  A slab of rows is staged FLAT into LDS (the global reads, and the read-modify-write of
// the vote buffer, are coalesced whatever P is), at a row stride of P | 1 words: thread t then scans row t of the slab, and the 32
// lanes of a half wave sit on 32 different banks.  The counters are integers in LDS; nothing is atomic in global memory and no
// floating-point value is ever accumulated across threads, so the result is a function of the inputs only.
// Launch-bound: Nt * (4 P + 8) bytes read, 8 Nt written with predictions (+ 8 Nt P with votes) -- 32 768 rows x 50 classes:
// 6.8 MB read + 0.26 MB written = ~7 MB (19.9 MB with votes), 1-3 us of HBM time at 8 TB/s against a ~6 us launch.
#include "common.h"
#include "eval_math.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_SLAB = 12288;                // floats of a row slab: 48 KiB of the 64 KiB a workgroup gets statically

struct EvalArgs {
    const float* logits; float* votes; const int64_t* y; const int32_t* ptr;
    const float* cat; const int32_t* part_start; const int32_t* part_count;
    int64_t* pred; double* iou; int32_t* hit; int32_t* cnt; int32_t* ignored;
    long long ld, Nt;
    int P, Cc;
};

__global__ __launch_bounds__(EV_THREADS) void eval_metrics_kernel(EvalArgs a) {
    __shared__ float slab[EV_SLAB];
    __shared__ int s_hit[dceval::MAX_P], s_cnt[dceval::MAX_P], s_npred[dceval::MAX_P];
    __shared__ int s_ign;
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, PS = P | 1;
    for (int c = tid; c < P; c += EV_THREADS) s_hit[c] = s_cnt[c] = s_npred[c] = 0;
    if (tid == 0) s_ign = 0;
    // the cloud's rows, held inside [0, Nt] whatever the offsets say
    long long r0 = a.ptr[b], r1 = a.ptr[b + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.Nt ? a.Nt : r0);
    r1 = r1 < r0 ? r0 : (r1 > a.Nt ? a.Nt : r1);
    const int rows_slab = EV_SLAB / PS < EV_THREADS ? EV_SLAB / PS : EV_THREADS;      // >= 47 (P = 256)
    const int dr = EV_THREADS / P, dc = EV_THREADS - dr * P;                          // one stride of 256 elements in (row, column)
    for (long long base = r0; base < r1; base += rows_slab) {
        const int nr = r1 - base < rows_slab ? (int)(r1 - base) : rows_slab;
        const int ne = nr * P;
        __syncthreads();                       // the counters are zero / the scan of the slab before is over
        int r = tid / P, c = tid - r * P;
        for (int e = tid; e < ne; e += EV_THREADS) {
            const long long row = base + r;
            float v = a.logits[row * a.ld + c];
            if (a.votes) {
                float* vp = a.votes + row * P + c;
                v = *vp + v;
                *vp = v;
            }
            slab[r * PS + c] = v;
            r += dr; c += dc;
            if (c >= P) { c -= P; ++r; }
        }
        __syncthreads();
        if (tid < nr) {
            const int idx = dceval::argmax_row(slab + tid * PS, P);
            const long long row = base + tid;
            if (a.pred) a.pred[row] = idx;
            atomicAdd(&s_npred[idx], 1);
            const long long y = a.y[row];
            if (y >= 0 && y < P) {             // a label outside [0, P) indexes nothing
                atomicAdd(&s_cnt[y], 1);
                if (y == idx) atomicAdd(&s_hit[y], 1);
            } else {
                atomicAdd(&s_ign, 1);
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < P; c += EV_THREADS) {
        a.hit[(long long)b * P + c] = s_hit[c];
        a.cnt[(long long)b * P + c] = s_cnt[c];
    }
    if (tid == 0) {
        a.ignored[b] = s_ign;
        if (a.iou) {
            int start = 0, count = P;
            if (a.cat) {
                const int k = dceval::argmax_row(a.cat + (long long)b * a.Cc, a.Cc);
                start = a.part_start[k];
                count = a.part_count[k];
            }
            a.iou[b] = dceval::iou_fold(s_hit, s_cnt, s_npred, P, start, count);
        }
    }
}

}  // namespace

// logits [Nt,P] with row stride ld_logits >= P (elements); votes null or [Nt,P] contiguous; y [Nt]; ptr [B+1] with values in
// [0, Nt] (values outside are clamped); category null or [B,Cc] with part_start / part_count [Cc] on the DEVICE; pred / iou may be
// null; hit / cnt [B,P], ignored [B].
DC_EXPORT int dc_eval_metrics(const float* logits, int64_t ld_logits, float* votes, const int64_t* y, const int32_t* ptr,
                              int32_t B, int64_t Nt, int32_t P, const float* category, int32_t Cc, const int32_t* part_start,
                              const int32_t* part_count, int64_t* pred, double* iou, int32_t* hit, int32_t* cnt, int32_t* ignored,
                              void* stream) {
    DC_REQUIRE(B >= 0 && Nt >= 0 && Cc >= 0, "dc_eval_metrics: negative size");
    DC_REQUIRE(P >= 1 && P <= dceval::MAX_P, "dc_eval_metrics: P = %d classes per row, supported: 1 .. %d", P, dceval::MAX_P);
    if (B == 0) return DC_OK;
    DC_REQUIRE(ptr && hit && cnt && ignored, "dc_eval_metrics: null pointer (ptr, hit, cnt, ignored)");
    DC_REQUIRE(Nt == 0 || (logits && y), "dc_eval_metrics: null pointer (logits, y)");
    DC_REQUIRE(ld_logits >= P, "dc_eval_metrics: row stride %lld of logits below P = %d", (long long)ld_logits, P);
    DC_REQUIRE(Nt < 2147483647L, "dc_eval_metrics: Nt < 2^31 rows (ptr is int32)");
    DC_REQUIRE(!category || (Cc > 0 && part_start && part_count), "dc_eval_metrics: categories need Cc > 0 and the two part tables");
    EvalArgs a;
    a.logits = logits; a.votes = votes; a.y = y; a.ptr = ptr; a.cat = category; a.part_start = part_start; a.part_count = part_count;
    a.pred = pred; a.iou = iou; a.hit = hit; a.cnt = cnt; a.ignored = ignored;
    a.ld = ld_logits; a.Nt = Nt; a.P = P; a.Cc = Cc;
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(B), dim3(EV_THREADS), 0, static_cast<hipStream_t>(stream), a);
    DC_CHECK_LAUNCH("dc_eval_metrics");
    return DC_OK;
}
