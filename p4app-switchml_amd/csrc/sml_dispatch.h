// sml_dispatch.h — runtime values -> compile-time constants, once, for every
// kernel launch site.  Each helper hands std::integral_constants to a generic
// lambda, which spells the kernel's template arguments from them by name:
//   dispatch_packet(P, [&](auto Pc) {
//       dispatch_bools([&](auto AL, auto BE) {
//           k<Pc(), AL(), BE()><<<grid, block, 0, st>>>(a);
//       }, al, be);
//   });
// The helpers are cartesian; a launch site that must not instantiate a
// combination folds it away inside the lambda (a constexpr value or
// `if constexpr`), with a comment saying why it cannot occur.
// No HIP here: plain C++17, so a host compiler can test it on its own.
#ifndef SML_DISPATCH_H_
#define SML_DISPATCH_H_

#include <stdint.h>

#include <type_traits>

namespace sml {

template <int N>
using int_c = std::integral_constant<int, N>;

// Packet size: 64 / 128 / 256 / 512, anything else 1024 (callers have
// checked valid_packet).
template <class F>
inline void dispatch_packet(uint32_t P, F&& f) {
    switch (P) {
        case 64:   f(int_c<64>{}); break;
        case 128:  f(int_c<128>{}); break;
        case 256:  f(int_c<256>{}); break;
        case 512:  f(int_c<512>{}); break;
        default:   f(int_c<1024>{}); break;
    }
}

// Tile slices: the listed value equal to U, anything else the last listed.
template <int U0, int... Us, class F>
inline void dispatch_slices(uint32_t U, F&& f) {
    if constexpr (sizeof...(Us) == 0) f(int_c<U0>{});
    else if (U == (uint32_t)U0) f(int_c<U0>{});
    else dispatch_slices<Us...>(U, f);
}

// Flags: f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...), in the
// order given.
template <class F>
inline void dispatch_bools(F&& f) { f(); }

template <class F, class... Rest>
inline void dispatch_bools(F&& f, bool b, Rest... rest) {
    if (b) dispatch_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else dispatch_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

}  // namespace sml

#endif  // SML_DISPATCH_H_
