// nd_amd/csrc/dispatch.hpp -- from a run-time value to a template argument, written once.  The launch sites of
// the omnibus units name a kernel instantiation through these three helpers: the callback is a generic lambda
// that receives the chosen value as a std::integral_constant, so `decltype(K)::value` is a constant expression
// inside it.  The lambda's body is instantiated for EVERY value of the list: an instantiation that must not
// exist (a series length float64 has no register form for, say) goes behind `if constexpr`, never a run-time
// `if`.  Plain C++17: no HIP header, so it compiles and is checked on a CPU (tests/test_dispatch_cpu.py).
#pragma once

#include <type_traits>

namespace nd_amd {

template <int V>
using int_c = std::integral_constant<int, V>;
template <bool V>
using bool_c = std::integral_constant<bool, V>;

// f(int_c<V>{}) for the FIRST V of the ascending list Vs with v <= V; false, and no call, if v is beyond the last
template <int... Vs, class F>
bool pick_le(int v, F &&f)
{
    return ((v <= Vs ? (f(int_c<Vs>{}), true) : false) || ...);
}

// f(int_c<V>{}) for the V of the list that equals v; false, and no call, if none does
template <int... Vs, class F>
bool pick_eq(int v, F &&f)
{
    return ((v == Vs ? (f(int_c<Vs>{}), true) : false) || ...);
}

// f(bool_c<b>{})
template <class F>
void pick(bool b, F &&f)
{
    if (b)
        f(bool_c<true>{});
    else
        f(bool_c<false>{});
}

}  // namespace nd_amd
