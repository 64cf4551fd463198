// lh_dispatch.hpp -- run-time facts made compile-time constants: the one way a launcher picks a kernel
// variant.  A launcher normalises its flags, nests these calls, and guards the combinations that have no
// kernel with `if constexpr` on a named predicate kept beside the kernel.
#pragma once
#include <type_traits>
#include <utility>

namespace lh {

template <int I> using int_c = std::integral_constant<int, I>;
template <int... Is> using int_list = std::integer_sequence<int, Is...>;
template <typename T> struct type_c { using type = T; }; // a type as a value (a math policy, a working type)

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
inline void with_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// f(int_c<I>{}) for the I of the list equal to v; the list's last value also stands for every v that
// is not in it, like a switch's default
template <int I0, int... Is, typename F>
inline void with_int(int_list<I0, Is...>, int v, F&& f) {
    if constexpr (sizeof...(Is) == 0) f(int_c<I0>{});
    else if (v == I0) f(int_c<I0>{});
    else with_int(int_list<Is...>{}, v, f);
}

} // namespace lh
