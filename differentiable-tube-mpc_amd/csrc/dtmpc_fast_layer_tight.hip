// dtmpc_fast_layer_tight.hip -- the backward of the differentiable solve under a per-trajectory constraint tightening
// and its row w.r.t. that tightening (dtmpc_solve_backward_tight, solve_backward_kernel<LKT, M, TRACK, W>: 32
// kernels) as a translation unit of its own, compiled in parallel with csrc/dtmpc_fast_layer.hip's 64 and
// csrc/dtmpc_fast_layer_dbas.hip's 32.  The text is dtmpc_fast_layer.hip's: its device part as it is, its host part
// with this family's block as the unit's (UnitBlocks) and the family's two entry points.
#define DTMPC_FAST_LAYER_TIGHT_TU 1
#include "dtmpc_fast_layer.hip"
