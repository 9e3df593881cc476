// Run-time values to compile-time constants, for the launchers: a generic lambda receives each value as a
// std::integral_constant (its template argument is the constant's call, k<K(), XF()>), and if constexpr on
// the constants inside the lambda keeps a kernel's instantiations to the combinations that exist.
// Host only, standard library only.
#pragma once

#include <type_traits>
#include <utility>

namespace cdfem {

// f(std::integral_constant<., V>{}) for the listed V that equals v; miss, and no call, when none does:
//   dispatch_value<3, 5>(c->p, hipErrorInvalidValue, [&](auto P) { return launch<P()>(c); })
template <auto V0, auto... Vs, class T, class R, class F>
R dispatch_value(T v, R miss, F &&f)
{
    if (v == static_cast<T>(V0)) return f(std::integral_constant<decltype(V0), V0>{});
    if constexpr (sizeof...(Vs) > 0) return dispatch_value<Vs...>(v, std::move(miss), std::forward<F>(f));
    else return miss;
}

// the operator's terms (CDFEM_DIFFUSION | CDFEM_CONVECTION | CDFEM_MASS): every non-empty mask
template <class R, class F>
R dispatch_kinds(unsigned kinds, R miss, F &&f)
{
    return dispatch_value<1u, 2u, 3u, 4u, 5u, 6u, 7u>(kinds, std::move(miss), std::forward<F>(f));
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...), the flags in the order written, f last:
//   dispatch_bools(x != nullptr, full, [&](auto XF, auto FU) { ... k<XF(), FU()> ... })
// (Bs: the flags already turned into constants; callers leave it empty)
template <bool... Bs, class F>
decltype(auto) dispatch_bools(F &&f)
{
    return std::forward<F>(f)(std::bool_constant<Bs>{}...);
}
template <bool... Bs, class... Rest>
decltype(auto) dispatch_bools(bool b, Rest &&...rest)
{
    return b ? dispatch_bools<Bs..., true>(std::forward<Rest>(rest)...)
             : dispatch_bools<Bs..., false>(std::forward<Rest>(rest)...);
}

}  // namespace cdfem
