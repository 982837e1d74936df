// dtmpc_fast_scenes.hip — the fused f32 solvers with per-trajectory scenes (dtmpc_tube_state.scenes,
// dtmpc_ilqr_solve_scenes): dtmpc_fast.hip's tube step and standalone iLQR instantiated with kScene, so every
// trajectory reads its own obstacle table and nominal target at each phase start.  A translation unit of its
// own, compiled in parallel with the shared-table units (the host part is the DTMPC_FAST_SCENES_TU branch there).
#define DTMPC_FAST_SCENES_TU 1
#include "dtmpc_fast.hip"
