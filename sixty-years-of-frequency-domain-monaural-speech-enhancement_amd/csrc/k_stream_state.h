// The row gather of se_stream_state_join (k_stream_state.hip): the gather of se_stream_state_select / _concat (kernels.h GatherArgs),
// except that in segment `seg` (the input window, outer == 1) a row of part p is part_inner[p] floats long and the destination row
// starts at its column part_col[p] - parts saved with live windows of different lengths, trimmed to one.
// part_col[p] + the destination's inner <= part_inner[p] is the caller's duty (stream_join.h: snap_join_plan).
#pragma once
#include "kernels.h"

namespace se {

struct JoinWindow {
    int seg = -1;
    const int* part_inner = nullptr;
    const int* part_col = nullptr;
    // tracking-scale streams (stream_join.h): segments [ring_lo, ring_hi) are per-frame rings [B][inner], inner a power of two, and
    // entry i of a row of part p comes from its entry (i - part_rot[p]) & (inner - 1); ring_lo >= ring_hi: none
    int ring_lo = 0, ring_hi = 0;
    const int* part_rot = nullptr;
    // per-row frame origins (stream_join.h): segment `origin_seg` is [Bd] int32, and a row of part p arrives as its value +
    // part_frames[p]; origin_seg < 0: none
    int origin_seg = -1;
    const int* part_frames = nullptr;
};
void launch_stream_state_join(const GatherArgs& a, const JoinWindow& w, long tiles, hipStream_t s);

}  // namespace se
