// The grid build of knn_grid.hip (box, zero, count, sum / scan, fill) for another translation unit of the library: fps_grid.hip
// samples over the same grids, cell starts and cell-ordered points.  Hidden symbols (the library exports only DC_EXPORT entries).
#pragma once
#include "common.h"
#include "knn_grid_math.h"

// What the build leaves in the workspace.  Cell c of cloud b, whose first row lies `off` rows behind the call's first row, is row
// 2 * off + b + c of `cell_start`; cell_start[row] .. cell_start[row + 1] are its slots of `pts` (entry `cells` of a cloud is the
// first slot of the next cloud).  A cloud that does not lie inside `cap` rows is built as an empty one (Grid.m = 0, one cell).
struct DcGridBuild {
    const dcgrid::Grid* grids;                // [B]
    const int64_t* cell_start;                // [2 cap + B + 1]
    const dcgrid::Pt* pts;                    // [cap], in cell order
    long long cap, rows;                      // points the workspace was carved for; 2 cap + B
};

// bytes of the build's workspace for `num_points` points in `num_clouds` clouds (dc_knn_grid_workspace_bytes)
size_t dc_grid_build_bytes(long long num_points, long long num_clouds);
// the largest point count whose build fits `bytes` (-1: not even an empty call)
long long dc_grid_build_capacity(size_t bytes, long long num_clouds);
// the five build launches over int64 offsets, carved for `cap` points at `workspace` (16-byte aligned) -> DC_OK or a launch error
int dc_grid_build(const char* name, const float* pos, const int64_t* ptr, int B, float target, void* workspace, long long cap,
                  hipStream_t stream, DcGridBuild* out);
