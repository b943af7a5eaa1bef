// ilu.hpp — what the check and the factor launches of g4s_ilu0 share (ilu.hip), in plain C++ (no HIP): the state block of the opening
// check, and the rule that spreads the rows of a level launch over its threads — it decides who factorises a row, never how: the bits of
// include/g4s.h do not depend on it.
#pragma once
#include "g4s.h"
namespace g4s {

// The state block of the opening check. The three rows are n while no row offends.
struct IluState {
    int invalid;          // 1: rowptr does not start at 0 or decreases
    int bad_id_row;       // the smallest row with an id outside [0, n)
    int bad_order_row;    // the smallest row whose ids are in range and do not ascend strictly
    int bad_diag_row;     // the smallest row that is neither and stores no diagonal entry
    int nnz_in;           // rowptr[n]
};

// How far apart the threads that own a row sit in a level launch (a power of two, 1 … 64): a level of `rows` rows whose strictly lower triangle
// holds `lower_entries` entries. A row's k loop is sequential and every step of it waits for a load, so rows are spread over waves sooner than the
// solve spreads them (trsv_stride): from one pivot a row on, twice as far per doubling, one wave a row from 64.
inline int ilu_stride(int rows, long long lower_entries)
{
    const long long avg = rows > 0 ? lower_entries / rows : 0;
    int s = 1;
    while (s < 64 && s <= avg) s *= 2;
    return s;
}

} // namespace g4s
