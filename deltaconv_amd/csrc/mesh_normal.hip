// Per-vertex normals of a device-resident store of triangle meshes -- replaces torch_geometric.transforms.GenerateMeshNormals as the
// reference's ShapeSeg pre_transform calls it once per shape on the host (experiments/train_shapeseg.py:31): an index_add_ of the
// face normals onto their corners (floating-point atomics on a device), then F.normalize.  Here the sum of a vertex is an ORDERED
// walk over its incident face corners: no floating-point atomics anywhere, the same bits on every run and on the host
// (csrc/mesh_normal_math.h, shared with tests/hostcheck_mesh_normal).
//
//   vertex_faces_*_kernel  the vertex-to-incident-corner lists of a whole store, built once: the shape of the in-edge lists of
//                          interp.hip (and of csc.hip).  One thread per corner slot e = 3 * face_row + corner: count (integer
//                          atomics on the vertex counters), exclusive scan over ALL vertex rows (list_scan.h), unordered fill
//                          (integer cursors), then the ranking: one fill position per thread, it finds its list through its
//                          corner's vertex and counts the smaller entries of that list.  The L^2 comparisons of a hub vertex's
//                          list are thus spread over the grid, L a thread.  The lists come out in ascending e whatever order the
//                          atomics ran in: a function of the inputs only.
//   vertex_normals_kernel  one vertex per thread on a flat grid over the vertex rows; the thread finds its mesh by bisection of
//                          vptr, walks its list in order and RECOMPUTES the contribution of every incident face from the three
//                          vertex rows.  The other form -- a first launch that writes the contributions [Fs,3] for this one to
//                          gather -- gives the same bits and a third of the arithmetic, but moves 24 more bytes per face through
//                          HBM (12 written, 12 read back), while the vertex rows a recomputation re-reads (about six times each)
//                          are a mesh's own and sit in L2: per face 24 (list) + 12 (ids) and per vertex 8 + 12 + 12 bytes of
//                          algorithmic traffic, in one launch and without a workspace.  The arithmetic (a cross product, a
//                          square root, a division per corner) is far from the VALU bound of a gather-bound kernel.  A thread's
//                          cost is its list length: a hub vertex with thousands of faces is walked by one thread -- correct, slow.
//                          The per-mesh count of zero normals is an integer atomic on a counter: order-free.
#include "common.h"
#include "list_scan.h"
#include "mesh_normal_math.h"

namespace {

constexpr int VN_THREADS = 256;
constexpr long long VN_MAX_SLOTS = (1ll << 31) * VN_THREADS - VN_THREADS;     // one thread per slot: at most 2^31 - 1 blocks
constexpr long long VN_MAX_VERTS = (1ll << 31) * VN_THREADS - VN_THREADS;     // (the scan's grid of 1024 rows reaches further)

__global__ __launch_bounds__(VN_THREADS) void vertex_faces_count_kernel(const int32_t* __restrict__ face,
                                                                        const int64_t* __restrict__ vptr,
                                                                        const int64_t* __restrict__ fptr, int B, long long num_verts,
                                                                        long long ne, u64* __restrict__ cnt) {
    const long long e = (long long)blockIdx.x * VN_THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long v = dcvnorm::corner_vertex(face, vptr, fptr, B, num_verts, e);
    if (v >= 0) atomicAdd(cnt + v, 1ull);
}

__global__ __launch_bounds__(VN_THREADS) void vertex_faces_fill_kernel(const int32_t* __restrict__ face,
                                                                       const int64_t* __restrict__ vptr,
                                                                       const int64_t* __restrict__ fptr, int B, long long num_verts,
                                                                       long long ne, u64* __restrict__ cursor,
                                                                       int64_t* __restrict__ unordered) {
    const long long e = (long long)blockIdx.x * VN_THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long v = dcvnorm::corner_vertex(face, vptr, fptr, B, num_verts, e);
    if (v < 0) return;
    const u64 at = atomicAdd(cursor + v, 1ull);
    if (at < (u64)ne) unordered[at] = e;      // (always: the counts came from the same inputs)
}

__global__ __launch_bounds__(VN_THREADS) void vertex_faces_rank_kernel(const int32_t* __restrict__ face,
                                                                       const int64_t* __restrict__ vptr,
                                                                       const int64_t* __restrict__ fptr, int B, long long num_verts,
                                                                       long long ne, const int64_t* __restrict__ vf_ptr,
                                                                       const int64_t* __restrict__ unordered,
                                                                       int64_t* __restrict__ vf_edge) {
    const long long t = (long long)blockIdx.x * VN_THREADS + threadIdx.x;
    if (t >= ne || t >= vf_ptr[num_verts]) return;
    const long long e = unordered[t];
    if (e < 0 || e >= ne) return;
    const long long v = dcvnorm::corner_vertex(face, vptr, fptr, B, num_verts, e);
    if (v < 0) return;
    long long lo = vf_ptr[v], hi = vf_ptr[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > ne ? ne : hi;
    long long rank = 0;
#pragma unroll 8
    for (long long p = lo; p < hi; ++p) rank += unordered[p] < e;
    if (lo + rank >= hi) return;              // (never: e is one of the list's distinct entries)
    vf_edge[lo + rank] = e;
}

__global__ __launch_bounds__(VN_THREADS) void vertex_normals_kernel(const float* __restrict__ vert, const int32_t* __restrict__ face,
                                                                    const int64_t* __restrict__ vptr,
                                                                    const int64_t* __restrict__ fptr, int B, long long num_verts,
                                                                    long long ne, const int64_t* __restrict__ vf_ptr,
                                                                    const int64_t* __restrict__ vf_edge, int weighting,
                                                                    float* __restrict__ normals, int32_t* __restrict__ zero_count) {
    const long long v = (long long)blockIdx.x * VN_THREADS + threadIdx.x;
    if (v >= num_verts) return;
    const int b = dcinterp::pair_of(vptr, B, v);
    if (b < 0) return;                        // a row outside every mesh of the call is not written
    const long long vbase = vptr[b];
    long long nv = vptr[b + 1] - vbase;
    if (vbase + nv > num_verts) nv = num_verts - vbase;          // nothing past vert [num_verts, 3] is read
    const long long fbase = fptr[b];
    long long nf = fptr[b + 1] - fbase;
    if (fbase < 0 || 3 * fbase > ne) nf = 0;  // nothing of this mesh lies inside face [ne / 3, 3]
    else if (3 * (fbase + nf) > ne) nf = ne / 3 - fbase;
    long long lo = vf_ptr[v], hi = vf_ptr[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > ne ? ne : hi;
    float n[3];
    const bool zero = dcvnorm::vertex_normal(vert, face, vbase, nv, fbase, nf, vf_edge + lo, hi > lo ? hi - lo : 0, weighting, n);
    normals[3 * v] = n[0];
    normals[3 * v + 1] = n[1];
    normals[3 * v + 2] = n[2];
    if (zero && zero_count) atomicAdd(zero_count + b, 1);
}

size_t vertex_faces_bytes(long long num_verts, long long num_faces) {
    return 8 * ((size_t)num_verts + (size_t)dc_cdiv(num_verts, SC_THREADS) + 3 * (size_t)num_faces);
}

}  // namespace

// workspace: the counters / fill cursors [num_verts], the scan's block sums and the unordered fill [3 * num_faces], 8 bytes each
DC_EXPORT size_t dc_mesh_vertex_faces_workspace_bytes(int64_t num_verts, int64_t num_faces) {
    if (num_verts < 0 || num_faces < 0 || num_verts > VN_MAX_VERTS || num_faces > VN_MAX_SLOTS / 3) return 0;
    return vertex_faces_bytes(num_verts, num_faces);
}

DC_EXPORT int dc_mesh_vertex_faces(const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B, int64_t num_verts,
                                   int64_t num_faces, int64_t* vf_ptr, int64_t* vf_edge, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    DC_REQUIRE(B >= 0, "dc_mesh_vertex_faces: B = %d meshes", B);
    DC_REQUIRE(num_verts >= 0 && num_verts <= VN_MAX_VERTS, "dc_mesh_vertex_faces: num_verts = %lld outside [0, 2^39)",
               (long long)num_verts);
    DC_REQUIRE(num_faces >= 0 && num_faces <= VN_MAX_SLOTS / 3, "dc_mesh_vertex_faces: num_faces = %lld: 3 * num_faces outside [0, 2^39)",
               (long long)num_faces);
    DC_REQUIRE(vf_ptr, "dc_mesh_vertex_faces: null pointer (vf_ptr)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long ne = 3 * (long long)num_faces;
    if (B == 0 || ne == 0 || num_verts == 0) {                   // no corner at all: every list is empty
        dc_zero_words(vf_ptr, 2 * ((long)num_verts + 1), s);
        DC_CHECK_LAUNCH("dc_mesh_vertex_faces");
        return DC_OK;
    }
    DC_REQUIRE(face && vptr && fptr && vf_edge, "dc_mesh_vertex_faces: null pointer (face, vptr, fptr, vf_edge)");
    DC_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= vertex_faces_bytes(num_verts, num_faces),
               "dc_mesh_vertex_faces: workspace null, not 8-byte aligned or too small (%zu bytes, needs %zu)", workspace_bytes,
               vertex_faces_bytes(num_verts, num_faces));
    const int sblocks = dc_cdiv(num_verts, SC_THREADS), eblocks = dc_cdiv(ne, VN_THREADS);
    u64* cnt = static_cast<u64*>(workspace);
    u64* part = cnt + num_verts;
    int64_t* unordered = reinterpret_cast<int64_t*>(part + sblocks);
    dc_zero_words(cnt, 2 * (long)num_verts, s);
    hipLaunchKernelGGL(vertex_faces_count_kernel, dim3(eblocks), dim3(VN_THREADS), 0, s, face, vptr, fptr, (int)B,
                       (long long)num_verts, ne, cnt);
    hipLaunchKernelGGL(list_sum_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_verts, part);
    hipLaunchKernelGGL(list_scan_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_verts, part, vf_ptr);
    hipLaunchKernelGGL(vertex_faces_fill_kernel, dim3(eblocks), dim3(VN_THREADS), 0, s, face, vptr, fptr, (int)B,
                       (long long)num_verts, ne, cnt, unordered);
    hipLaunchKernelGGL(vertex_faces_rank_kernel, dim3(eblocks), dim3(VN_THREADS), 0, s, face, vptr, fptr, (int)B,
                       (long long)num_verts, ne, vf_ptr, unordered, vf_edge);
    DC_CHECK_LAUNCH("dc_mesh_vertex_faces");
    return DC_OK;
}

DC_EXPORT int dc_mesh_vertex_normals(const float* vert, const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B,
                                     int64_t num_verts, int64_t num_faces, const int64_t* vf_ptr, const int64_t* vf_edge,
                                     int32_t weighting, float* normals, int32_t* zero_count, void* stream) {
    DC_REQUIRE(B >= 0, "dc_mesh_vertex_normals: B = %d meshes", B);
    DC_REQUIRE(num_verts >= 0 && num_verts <= VN_MAX_VERTS, "dc_mesh_vertex_normals: num_verts = %lld outside [0, 2^39)",
               (long long)num_verts);
    DC_REQUIRE(num_faces >= 0 && num_faces <= VN_MAX_SLOTS / 3, "dc_mesh_vertex_normals: num_faces = %lld: 3 * num_faces outside [0, 2^39)",
               (long long)num_faces);
    DC_REQUIRE(weighting == dcvnorm::W_UNIFORM || weighting == dcvnorm::W_AREA,
               "dc_mesh_vertex_normals: weighting = %d, supported: 0 (uniform) and 1 (area)", weighting);
    if (B == 0 || num_verts == 0) return DC_OK;
    DC_REQUIRE(vert && face && vptr && fptr && vf_ptr && normals,
               "dc_mesh_vertex_normals: null pointer (vert, face, vptr, fptr, vf_ptr, normals)");
    DC_REQUIRE(num_faces == 0 || vf_edge, "dc_mesh_vertex_normals: null pointer (vf_edge)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (zero_count) dc_zero_words(zero_count, (long)B, s);
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(dc_cdiv(num_verts, VN_THREADS)), dim3(VN_THREADS), 0, s, vert, face, vptr, fptr,
                       (int)B, (long long)num_verts, 3 * (long long)num_faces, vf_ptr, vf_edge, (int)weighting, normals, zero_count);
    DC_CHECK_LAUNCH("dc_mesh_vertex_normals");
    return DC_OK;
}
