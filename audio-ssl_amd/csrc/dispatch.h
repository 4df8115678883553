// Host-side dispatch from the C ABI's integer codes to template instantiations (C++17; nothing from HIP but __bf16).
#pragma once
#include <type_traits>

typedef __bf16 bf16;
template <typename T> struct TypeTag { using type = T; };

// The storage-type rule of every launcher: `dtype` is the path's type (0 = fp32, 1 = bf16); each further code belongs to a
// "wide" tensor that may stay fp32 on the bf16 path and is 0 or equal to `dtype` (the entry point has validated that).
// assl_dispatch calls the generic lambda `f` with one tag for the path and one per wide code: all float when dtype == 0,
// else bf16 followed by float where the code is 0 and bf16 elsewhere.  f is instantiated for those 1 + 2^n tuples only
// (2, 3 or 5 kernels), in the order FF.., BFF, BFB, BBF, BBB - never for the cross product of the codes.
template <typename... Done> struct AsslWide {
    template <typename F> static void go(F& f) { f(Done{}...); }
    template <typename F, typename... W> static void go(F& f, int code, W... rest) {
        if (code == 0) AsslWide<Done..., TypeTag<float>>::go(f, rest...);
        else           AsslWide<Done..., TypeTag<bf16>>::go(f, rest...);
    }
};
template <typename F, typename... W> inline void assl_dispatch(int dtype, F&& f, W... wide) {
    static_assert((std::is_same_v<W, int> && ...), "wide codes are ints");
    if (dtype == 0) f(TypeTag<float>{}, ((void)wide, TypeTag<float>{})...);
    else            AsslWide<TypeTag<bf16>>::go(f, wide...);
}
// Rows per thread of the one-launch BatchNorm / centering kernels: 8 up to 512 rows per group, 16 up to their limit of 1024.
template <typename F> inline void assl_rows(long M, F&& f) {
    if (M <= 512) f(std::integral_constant<int, 8>{});
    else          f(std::integral_constant<int, 16>{});
}

#ifdef __HIP__      // launch helpers: they name HIP types, a plain C++ translation unit gets the dispatch above alone
inline hipStream_t S_(void* stream) { return static_cast<hipStream_t>(stream); }
inline dim3 GRID1(long n) { return dim3((unsigned)((n + 255) / 256)); }
#endif
