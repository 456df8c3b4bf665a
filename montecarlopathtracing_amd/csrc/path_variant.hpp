// The variants the path kernels are compiled in -- with or without an environment (ENV), times the light-pick mode (PICK: 0 every
// light, 1 MCPT_LIGHTS_ONE, 2 MCPT_LIGHTS_TREE) -- and the one place where a scene's run-time state becomes those template arguments.
// Host code; every launcher of a <ENV, PICK> kernel goes through with_path_variant, and LaunchCfg's per-variant arrays are indexed by
// variant_index.  A new mode is a new case here.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "device_scene.hpp"

namespace mcpt {

constexpr int kPickModes = 3;                       // pick_mode(): 0, 1, 2
constexpr int kPathVariants = 2 * kPickModes;
constexpr int variant_index(bool env, int pick) { return pick * 2 + (env ? 1 : 0); }

// f(env, pick) with the variant as types: env() is a constexpr bool, pick() a constexpr int.  A pick mode without a case here has no
// kernels: an error, not a launch of some other variant's.
template <class F>
inline void with_path_variant(bool env, int pick, F&& f)
{
    using std::integral_constant;
    switch (variant_index(env, pick)) {
    case variant_index(false, 0): f(std::false_type{}, integral_constant<int, 0>{}); break;
    case variant_index(true, 0): f(std::true_type{}, integral_constant<int, 0>{}); break;
    case variant_index(false, 1): f(std::false_type{}, integral_constant<int, 1>{}); break;
    case variant_index(true, 1): f(std::true_type{}, integral_constant<int, 1>{}); break;
    case variant_index(false, 2): f(std::false_type{}, integral_constant<int, 2>{}); break;
    case variant_index(true, 2): f(std::true_type{}, integral_constant<int, 2>{}); break;
    default: std::fprintf(stderr, "mcpt: no path kernels for light-pick mode %d\n", pick); std::abort();
    }
}
template <class F>
inline void with_path_variant(const DScene& S, F&& f) { with_path_variant(env_on(S.env), pick_mode(S.pick), f); }
// every variant in turn (what is set up once per device for each of them)
template <class F>
inline void for_each_path_variant(F&& f)
{
    for (int pick = 0; pick < kPickModes; pick++)
        for (int env = 0; env < 2; env++) with_path_variant(env != 0, pick, f);
}

}  // namespace mcpt
