// dtmpc_fast_layer_dbas.hip -- the differentiable solve's rows w.r.t. the DBaS parameters alpha and gamma
// (dtmpc_solve_backward_dbas, solve_backward_kernel<LKD, M, TRACK, W>: 32 kernels) as a translation unit of its own,
// compiled in parallel with csrc/dtmpc_fast_layer.hip's 64.  The text is that file's: its device part as it is, its
// host part with this family's block as the unit's (UnitBlocks) and the family's two entry points.
#define DTMPC_FAST_LAYER_DBAS_TU 1
#include "dtmpc_fast_layer.hip"
