// The one place that turns (d, elem_bytes) into a compile-time width and element type: with_pair<Set>(d, elem_bytes, f) calls
// f(std::integral_constant<int, D>(), (T*)nullptr) for a pair the set admits and returns true; any other pair: nothing is called,
// false -- the launchers' refusal (hipErrorInvalidValue), the host walks' false, and what the sml_*_supports functions answer.
// A set names the widths admitted per element type as the bit-OR of the widths themselves (32, 64 and 128 are distinct powers of two;
// with_width_of refuses to compile for a width that is not, which would match other widths' bits).  They are compile-time parameters under
// `if constexpr`: a kernel named inside the generic callable is instantiated for the set's pairs only.
#ifndef SML_WIDTH_DISPATCH_H
#define SML_WIDTH_DISPATCH_H
#include <type_traits>

struct RetrievalPairs { static constexpr int f32 = 32 | 64, f16 = 32 | 64 | 128; };         // retrieval.hip, ivf.hip, rerank.hip
struct FoldInPairs { static constexpr int f32 = 32 | 64, f16 = 32 | 64; };                  // als.hip (d = 128 is out of scope)
struct PropagationPairs { static constexpr int f32 = 32 | 64 | 128, f16 = 32 | 64 | 128; }; // graph.hip: all six

template <int Widths, class T, int D, class Fn>
bool with_width_of(int d, Fn& f) {
    static_assert(D > 0 && (D & (D - 1)) == 0, "a set is a bit mask of widths: every width must be a power of two");
    if constexpr ((Widths & D) != 0) {
        if (d == D) { f(std::integral_constant<int, D>(), (T*)nullptr); return true; }
    }
    return false;
}

template <class Set, class Fn>
bool with_pair(int d, int elem_bytes, Fn&& f) {
    if (elem_bytes == 4)
        return with_width_of<Set::f32, float, 32>(d, f) || with_width_of<Set::f32, float, 64>(d, f) || with_width_of<Set::f32, float, 128>(d, f);
    if (elem_bytes == 2)
        return with_width_of<Set::f16, _Float16, 32>(d, f) || with_width_of<Set::f16, _Float16, 64>(d, f) || with_width_of<Set::f16, _Float16, 128>(d, f);
    return false;
}

#endif
