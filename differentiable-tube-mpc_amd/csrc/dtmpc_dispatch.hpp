// dtmpc_dispatch.hpp — host only: how the fused units map a runtime value onto one of their compile-time
// instantiations.  pick<1, 2, 4>(lanes, f) calls the generic callable f with the matching value as a
// std::integral_constant; picks nest, one per template argument of the kernel, with the launch in the innermost
// callable.  A combination a unit does not hold is kept out of its instantiation set with `if constexpr` on the
// constants there (the callable then returns false), never with a runtime test.
#pragma once

#include <cstdio>
#include <type_traits>

#include "dtmpc_host.hpp"

namespace dtmpc {

// f(c)'s own answer where it gives one, else true
template <class F, class C>
inline bool pick_call(F& f, C c) {
  if constexpr (std::is_void_v<decltype(f(c))>) {
    f(c);
    return true;
  } else {
    return f(c);
  }
}

// f(std::integral_constant<int, V>) for the V of the list equal to v; false when none is (or f itself returned false)
template <int... Vs, class F>
inline bool pick(int v, F&& f) {
  return ((v == Vs && pick_call(f, std::integral_constant<int, Vs>{})) || ...);
}
// ... and f(std::bool_constant<b>)
template <class F>
inline bool pick_flag(bool b, F&& f) {
  return b ? pick_call(f, std::true_type{}) : pick_call(f, std::false_type{});
}

// The obstacle counts the fused kernels are instantiated for.  -DDTMPC_FAST_M_ONLY=m builds only m (experiment
// variants of the library: an eighth of the compile time; other counts then return DTMPC_ERR_BAD_ARG).  ISA5: a unit
// that holds only five obstacles in an ISA inspection build (-DDTMPC_FAST_ISA_ONLY).
// (Descending, and the lists of the picks inside in the same sense: clang emits the kernels of a fold last first, so
// each unit's kernels keep the places in its code object that the former switch ladders gave them -- the f64 kernels
// reach sincos_far pc-relatively, their text depends on where they lie; scripts/isa_identity.py compares it.)
#ifdef DTMPC_FAST_M_ONLY
#define DTMPC_OBSTACLE_COUNTS DTMPC_FAST_M_ONLY
#else
#define DTMPC_OBSTACLE_COUNTS 8, 7, 6, 5, 4, 3, 2, 1
#endif
#if defined(DTMPC_FAST_ISA_ONLY) && !defined(DTMPC_FAST_M_ONLY)
constexpr bool kIsaFive = true;
#else
constexpr bool kIsaFive = false;
#endif
template <bool ISA5 = false, class F>
inline bool pick_obstacles(int M, F&& f) {
  if constexpr (ISA5 && kIsaFive) {
    return pick<5>(M, f);
  } else {
    return pick<DTMPC_OBSTACLE_COUNTS>(M, f);
  }
}

// what a launcher returns when a pick found nothing
inline int not_instantiated(const char* launcher) {
  char msg[128];
  std::snprintf(msg, sizeof(msg), "%s: obstacle count not instantiated", launcher);
  return set_err(DTMPC_ERR_BAD_ARG, msg);
}

}  // namespace dtmpc
