// dispatch.h -- runtime flags to template arguments.  Host-only, no HIP header: tests/test_dispatch_helper.py compiles it with g++.
//
//   with_bools([&](auto P2, auto KP) { return launch_lds(name, kernel<P2(), KP()>, ...); }, pow2, keep);
//   with_int<1, 2, 3, 4>(pmode, [&](auto M) { return launch_lds(name, kernel<M()>, ...); });
//
// Both instantiate `f` for the WHOLE product of their values: use them only where every combination is a kernel the library
// ships today, and spell a sparse choice out.
#pragma once
#include <type_traits>

#include "gdf/gdf.h"

namespace gdf_amd {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): the flags arrive in argument order
template <class F>
static inline gdf_error with_bools(F &&f) { return f(); }
template <class F, class... Rest>
static inline gdf_error with_bools(F &&f, bool b, Rest... rest) {
  auto bind = [&](auto B) { return with_bools([&](auto... Rs) { return f(B, Rs...); }, rest...); };
  return b ? bind(std::true_type{}) : bind(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; a value that is not on the list: GDF_INVALID_API_CALL, f not called
template <int... Vs, class F>
static inline gdf_error with_int(int v, F &&f) {
  gdf_error r = GDF_INVALID_API_CALL;
  (void)((v == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return r;
}

}  // namespace gdf_amd
