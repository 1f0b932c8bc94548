// Host-side rules shared by the three launchers of the GEMM family (gemm.hip, gemm_bf16.hip, gemm_x3.hip).
#pragma once
#include <type_traits>
#include "common.h"
#include "prof.h"
#include "roitr_engine.h"

// shapes the fused LayerNorm epilogue takes: one block spans the row (64 / 128 / 256 columns), no batching, no ReLU before the norm
static inline bool gemm_ln_shape_ok(const RoitrGemm* g)
{
    const int tn = g->N / 64;
    return g->N % 64 == 0 && (tn == 1 || tn == 2 || tn == 4) && g->batch == 1 && !g->seg_off && !g->relu && g->ln_beta;
}

// tiles of the launch; false: more than the 1-D grid takes (the refusal's text: GEMM_TOO_MANY_TILES)
#define GEMM_TOO_MANY_TILES "roitr_gemm: too many tiles for one grid (row tiles x column tiles x batch > 0x7ffffff0)"
static inline bool gemm_tile_count(int nx, int ny, int batch, int* T)
{
    const long Tl = (long)nx * ny * batch;
    if (Tl > 0x7ffffff0L) return false;
    *T = (int)Tl;
    return true;
}

// opens the profiler bracket of a launch (close it with roitr_prof_end on the returned class)
static inline int gemm_prof_begin(const RoitrGemm* g, hipStream_t stream)
{
    const int cls = roitr_prof_is_enabled() ? roitr_gemm_prof_class(g) : ROITR_PROF_GEMM;
    if (g->batch_live)   // priced on the LIVE batches (device-side count), not on the capacity of the list
        roitr_prof_begin_live(cls, 2.0 * g->M * g->N * (double)g->K, roitr_gemm_algorithmic_bytes(g) / g->batch, g->batch_live, stream);
    else roitr_prof_begin2(cls, 2.0 * g->M * g->N * (double)g->K * g->batch, roitr_gemm_algorithmic_bytes(g), stream);
    return cls;
}

// fn(std::integral_constant<int, TN>) for the tile width tn in {1, 2, 4}
template <class Fn>
void dispatch_tn(int tn, Fn fn)
{
    switch (tn) {
    case 1: fn(std::integral_constant<int, 1>()); break;
    case 2: fn(std::integral_constant<int, 2>()); break;
    default: fn(std::integral_constant<int, 4>()); break;
    }
}
