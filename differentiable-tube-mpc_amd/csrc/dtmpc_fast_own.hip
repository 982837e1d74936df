// dtmpc_fast_own.hip — the fused f32 tube step with per-trajectory ancillary weights ("own theta",
// dtmpc_tube_step_own): dtmpc_fast.hip's tube step instantiated with kOwn (and with kOwn | kScene), so every
// trajectory solves with its own column of theta [6][B] and updates it from its own gradient row at the end of the
// step.  A translation unit of its own, compiled in parallel with the shared-theta units (the host part is the
// DTMPC_FAST_OWN_TU branch there).
#define DTMPC_FAST_OWN_TU 1
#include "dtmpc_fast.hip"
