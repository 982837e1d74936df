// dtmpc_fast_weights.hip — the fused f32 standalone iLQR with per-trajectory cost weights (dtmpc_ilqr_solve_weights):
// dtmpc_fast.hip's ilqr_fast_kernel instantiated with kWts (and with kWts | kScene), so every trajectory solves with
// its own column of the weights array [9][B] -- and, with scenes, its own obstacle table and target.  A translation
// unit of its own, compiled in parallel with the shared-weights units (the host part is the DTMPC_FAST_WEIGHTS_TU
// branch there).
#define DTMPC_FAST_WEIGHTS_TU 1
#include "dtmpc_fast.hip"
