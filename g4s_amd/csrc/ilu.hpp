// ilu.hpp — the state block of the opening check of g4s_ilu0 (ilu.hip), in plain C++ (no HIP).
#pragma once
namespace g4s {

// The three rows are n while no row offends.
struct IluState {
    int invalid;          // 1: rowptr does not start at 0 or decreases
    int bad_id_row;       // the smallest row with an id outside [0, n)
    int bad_order_row;    // the smallest row whose ids are in range and do not ascend strictly
    int bad_diag_row;     // the smallest row that is neither and stores no diagonal entry
    int nnz_in;           // rowptr[n]
};

} // namespace g4s
