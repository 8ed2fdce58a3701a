// dispatch.h -- runtime selector -> template parameter, for the launch sites of both device translation units.  f is called once, with
// a std::integral_constant of the selected value, so that each branch is a plain launch of its own instantiation.
//   with_method(method, f)        METHOD 0 / 1 / 2 (validated by the callers; anything else runs as 2)
//   with_choice<A, B>(second, f)  a two-way parameter (source form, occlusion mode, index arithmetic, block shape): B if `second`, else A
//   with_int<Lo, Hi>(v, f)        one of Lo .. Hi; a value outside the range runs as the nearer end
#pragma once
#include <type_traits>
#include <utility>

template <class F>
void with_method(int method, F&& f) {
    if (method == 0) f(std::integral_constant<int, 0>{});
    else if (method == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
template <int A, int B, class F>
void with_choice(bool second, F&& f) {
    if (second) f(std::integral_constant<int, B>{});
    else f(std::integral_constant<int, A>{});
}
template <int Lo, class F, int... I>
void with_int_in_range(int v, F&& f, std::integer_sequence<int, I...>) {
    (void)((v == Lo + I && (f(std::integral_constant<int, Lo + I>{}), true)) || ...);
}
template <int Lo, int Hi, class F>
void with_int(int v, F&& f) {
    with_int_in_range<Lo>(v < Lo ? Lo : v > Hi ? Hi : v, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}
