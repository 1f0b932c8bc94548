// The per-cloud uniform grid of pointops_knn.hip, for the other sources that walk it (pairgt.hip).
// Built by roitr_knn_build_grid(_ex) into a roitr_knn_workspace_bytes workspace; the layout inside the workspace stays private to
// pointops_knn.hip, which hands out this view.
#pragma once
#include <hip/hip_runtime.h>

#define GRID_MAX_CELLS 16384
#define GRID_MAX_DIM 255

struct RoitrGrid {  // one per cloud
    float ox, oy, oz, h, inv_h;
    int nx, ny, nz;
};
// A point (x, y, z) of cloud c lies in cell (cz * ny + cy) * nx + cx with, per axis and in fp32,
//     cx = min(max((int)floorf((x - ox) * inv_h), 0), nx - 1)
// (grid_build_kernel); cell k of cloud c holds sorted[cell_start[c * (GRID_MAX_CELLS + 1) + k] .. cell_start[... + k + 1]), GLOBAL rows
// of `sorted`, whose entries are (x, y, z, original global row as int bits).  ox, oy, oz are the cloud's exact coordinate minima.
struct RoitrGridView {
    const RoitrGrid* grids;
    const int* cell_start;
    const float4* sorted;
};
// host only: the view of a workspace roitr_knn_build_grid was (or will be) called on with the same (b, n, m_capacity)
RoitrGridView roitr_knn_grid_view(int b, int n, int m_capacity, void* ws);
