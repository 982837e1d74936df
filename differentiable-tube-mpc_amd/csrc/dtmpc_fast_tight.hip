// dtmpc_fast_tight.hip — the fused f32 standalone iLQR with a per-trajectory constraint tightening
// (dtmpc_ilqr_solve_tight): dtmpc_fast.hip's ilqr_fast_kernel instantiated with kTight | kTightPT (and with kScene as
// well), so every trajectory's barrier sees h(x) - s_i with s_i its own element of the tight array [B] -- and, with
// scenes, its own obstacle table and target.  A translation unit of its own, compiled in parallel with the other
// standalone-iLQR units (the host part is the DTMPC_FAST_TIGHT_TU branch there).
#define DTMPC_FAST_TIGHT_TU 1
#include "dtmpc_fast.hip"
