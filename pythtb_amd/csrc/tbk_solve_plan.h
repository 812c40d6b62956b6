// tbk_solve_plan.h -- the launch arithmetic of the mesh solve that more than one driver shares: pure host functions, no device
// call (check/plan_check.cpp holds them to a table of the values the drivers computed before they were shared).
#pragma once
#include <stdint.h>
#include <algorithm>

// Wave tiles of a mesh row (k_grid_rows, k_grid_rows_flux).  A row is `cpr` chunks of 64 columns, a tile `seg` chunks of one row
// (or of one group of rows), `tpr` tiles per row.  seg: enough tiles to reach `want` over the `nrows` rows (or row groups), at most
// seg_cap and a whole row; TBK_GRID_SEG (`knob` >= 0) replaces it -- held to seg_cap where the cap is a hard limit (`knob_capped`:
// the fused kernel's LDS), to the row alone where it is a measured default (the row kernel).  Then the tiles of a row are
// balanced: 33 chunks at seg = 8 are 5 tiles of 7,7,7,7,5, not 8,8,8,8,1.
// Returns the number of tiles; *seg_out, *tpr_out.
static inline int64_t tbk_tile_balance(int cpr, int64_t nrows, int64_t want, int seg_cap, int knob, bool knob_capped, int* seg_out,
                                       int* tpr_out) {
    int seg = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(seg_cap, cpr), (int64_t)cpr * nrows / want));
    if (knob >= 0) seg = std::max(1, std::min(knob_capped ? std::min(knob, seg_cap) : knob, cpr));
    *tpr_out = (cpr + seg - 1) / seg;
    *seg_out = (cpr + *tpr_out - 1) / *tpr_out;
    return nrows * *tpr_out;
}

// Chains of `run` consecutive points along the last mesh axis, aligned to the GLOBAL index (k_solve_wave on a mesh): the chains
// that touch the window [off, off + nl) are as many as returned, from number *first on.
static inline int tbk_chunk_window(int64_t off, int64_t nl, int64_t run, int64_t* first) {
    *first = off / run;
    return (int)((off + nl - 1) / run - *first + 1);
}
