// ofl_median_net.h -- the sorting network of the median filter (K16), as a compile-time table.
//
// Batcher's odd-even merge sort in its iterative form, which holds for any N: the comparators of the network for the next
// power of two that touch an index >= N are left out -- those wires would carry +infinity and never move.  net_make<N>()
// lists the comparators (lo < hi, the smaller value goes to lo) in order; net_sort<N>(a) applies them to a register array
// with every index a constant, so nothing is indexed dynamically and what feeds only unused outputs is dead code the
// compiler removes (a caller that reads a[(N - 1) / 2] alone pays for a median network, not for a sort).
// Plain C++17 without any device construct of its own: tests/test_median_host.py compiles it for the host and checks it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>
#include <utility>

#if defined(__HIPCC__)
#define OFL_NET_FN __host__ __device__ __forceinline__
#else
#define OFL_NET_FN inline
#endif

namespace ofl {

// visit(lo, hi) for every comparator of the N-wire network, in order
template <int N, typename F>
constexpr void net_walk(F &&visit)
{
    for (int p = 1; p < N; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j + k < N; j += 2 * k)
                for (int i = 0; i < k && i + j + k < N; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) visit(i + j, i + j + k);
}

template <int N>
constexpr int net_count()
{
    int c = 0;
    net_walk<N>([&c](int, int) { ++c; });
    return c;
}

template <int N>
struct Net {
    static constexpr int count = net_count<N>();
    uint8_t lo[count], hi[count];
};

template <int N>
constexpr Net<N> net_make()
{
    Net<N> t{};
    int c = 0;
    net_walk<N>([&t, &c](int lo, int hi) { t.lo[c] = (uint8_t)lo; t.hi[c] = (uint8_t)hi; ++c; });
    return t;
}

template <int N> inline constexpr Net<N> kNet = net_make<N>();

template <int N, size_t I>
OFL_NET_FN void net_step(uint32_t (&a)[N])
{
    constexpr int lo = kNet<N>.lo[I], hi = kNet<N>.hi[I];
    static_assert(lo < hi && hi < N, "comparator");
    const uint32_t x = a[lo], y = a[hi];
    a[lo] = x < y ? x : y;
    a[hi] = x < y ? y : x;
}

template <int N, size_t... I>
OFL_NET_FN void net_apply(uint32_t (&a)[N], std::index_sequence<I...>)
{
    (void)std::initializer_list<int>{ (net_step<N, I>(a), 0)... };      // a braced list: evaluated left to right
}

// a[0] <= a[1] <= ... <= a[N - 1] as unsigned integers
template <int N>
OFL_NET_FN void net_sort(uint32_t (&a)[N])
{
    net_apply<N>(a, std::make_index_sequence<(size_t)Net<N>::count>());
}

}  // namespace ofl
