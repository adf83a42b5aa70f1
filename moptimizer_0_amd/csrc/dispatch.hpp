// Run-time value -> compile-time tag, handed to a generic lambda: the one place where a word of the
// C ABI (a covariance form, a Jacobian mode, a scalar width, a flag) becomes a template argument.
//
//   return dispatch::intOrFail<kJacAnalytic, kJacAnalyticTst>(jac_mode, hipErrorInvalidValue, [&](auto jac) {
//     return dispatch::byBool(site.streaming, [&](auto streaming) {
//       return launch(kernel<S, jac(), streaming()>, ...);
//     });
//   });
//
// The tag of an integer or a bool is a std::integral_constant (`jac()` is its value, a constant
// expression); the tag of a scalar type is a Type<T> (`typename decltype(tag)::type`).  Every call
// states what a value outside its list does: the tag of a named default, or a failure value of the
// caller's returned without running the lambda.  All lambdas of one call return the same type, and
// that is what the call returns.  Host code only: no HIP header, no project header.
#pragma once

#include <type_traits>

namespace mopt {
namespace dispatch {

template <int V>
using Int = std::integral_constant<int, V>;
template <typename T>
struct Type {
  using type = T;
};

// f(Int<V>{}) for the first V of First, Rest... that equals `value`; the last of the list takes every
// other value.  The return type comes from the first of the list and no callable of the caller's is
// wrapped on the way, so the lambda is instantiated in the order of the list — and the kernels it
// names are emitted in that order, which keeps a code object's layout a function of the lists alone.
template <int First, int... Rest, typename F>
auto intOrLast(int value, F &&f) -> decltype(f(Int<First>{})) {
  if constexpr (sizeof...(Rest) == 0) {
    return f(Int<First>{});
  } else {
    if (value == First) return f(Int<First>{});
    return intOrLast<Rest...>(value, f);
  }
}

// an unlisted value takes the tag of Default
template <int Default, int... Listed, typename F>
auto intOrDefault(int value, F &&f) {
  return intOrLast<Listed..., Default>(value, f);
}

// an unlisted value returns `failure`
template <int First, int... Rest, typename R, typename F>
R intOrFail(int value, R failure, F &&f) {
  if (value == First) return f(Int<First>{});
  if constexpr (sizeof...(Rest) > 0)
    return intOrFail<Rest...>(value, failure, f);
  else
    return failure;
}

template <typename F>
auto byBool(bool value, F &&f) -> decltype(f(std::true_type{})) {
  return value ? f(std::true_type{}) : f(std::false_type{});
}

// a scalar width in bytes: 8 -> Type<double>, 4 -> Type<float>; any other the tag of Default ...
template <typename Default, typename F>
auto widthOrDefault(int bytes, F &&f) -> decltype(f(Type<Default>{})) {
  if (bytes == 8) return f(Type<double>{});
  if (bytes == 4) return f(Type<float>{});
  return f(Type<Default>{});
}

// ... or `failure`
template <typename R, typename F>
R widthOrFail(int bytes, R failure, F &&f) {
  if (bytes == 8) return f(Type<double>{});
  if (bytes == 4) return f(Type<float>{});
  return failure;
}

}  // namespace dispatch
}  // namespace mopt
