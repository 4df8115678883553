// Drives csrc/dispatch.h on the CPU (tests/test_host_logic.py builds this with the address and undefined-behaviour
// sanitizers and compares the output): one line per call, the tags handed to the lambda as F (float) / B (bf16), then how
// many instantiations of the lambda the helper caused per number of tags (1 + 2^n; a cross product would give 2^(n+1)).
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "dispatch.h"

template <typename T> constexpr char letter() {
    static_assert(std::is_same_v<T, float> || std::is_same_v<T, bf16>, "a tag is float or bf16");
    return std::is_same_v<T, float> ? 'F' : 'B';
}

static int instances[4];
template <typename... T> struct Seen { static inline const bool counted = (++instances[sizeof...(T)], true); };
template <typename... Tag> void show(const char* codes) {
    (void)Seen<typename Tag::type...>::counted;
    const char tags[] = {letter<typename Tag::type>()..., 0};
    std::printf("d %s %s\n", codes, tags);
}

int main() {
    char codes[16];
    for (int dtype = 0; dtype < 2; ++dtype) {
        std::snprintf(codes, sizeof codes, "%d", dtype);
        assl_dispatch(dtype, [&](auto t) { show<decltype(t)>(codes); });
        for (int w1 = 0; w1 <= dtype; ++w1) {                      // every legal tuple: a wide code is 0 or dtype
            std::snprintf(codes, sizeof codes, "%d %d", dtype, w1);
            assl_dispatch(dtype, [&](auto t, auto a) { show<decltype(t), decltype(a)>(codes); }, w1);
            for (int w2 = 0; w2 <= dtype; ++w2) {
                std::snprintf(codes, sizeof codes, "%d %d %d", dtype, w1, w2);
                assl_dispatch(dtype, [&](auto t, auto a, auto g) { show<decltype(t), decltype(a), decltype(g)>(codes); }, w1, w2);
            }
        }
    }
    for (long M : {1L, 512L, 513L, 1024L})
        assl_rows(M, [&](auto nr) { std::printf("r %ld %d\n", M, nr()); });
    std::printf("i %d %d %d\n", instances[1], instances[2], instances[3]);
    return 0;
}
