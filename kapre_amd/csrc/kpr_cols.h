// kpr_cols.h -- the column-group vocabulary of the time-tiled kernels (k_pcen, k_cmvn, k_time_stretch): which columns a lane owns
// and how it moves them.  Part of the single translation unit kapre_hip.hip (right after kpr_common.h).
//
// The problem is a contiguous (outer, frames, inner) tensor that is scanned or reduced along `frames`.  A lane owns one column
// group: V consecutive inner indices of one outer item, moved with one access (V > 1: inner % V == 0 and bases aligned to the
// access; col_launch on the host decides), or a single column (V = 1).  Column groups are numbered through all outer items, so 64
// consecutive groups fill a wave whatever `inner` is, and a workgroup of W waves owns 64 of them.  Time is tiled: one step covers
// a super-block of W * R rows, wave w holding the R rows (sb W + w) R ... of super-block sb in registers.  A wave reduces its chunk
// from a neutral carry-in and leaves the result in LDS, indexed by lane; after ONE barrier every wave combines the W results in
// order, redundantly, and so holds its own carry-in and the state after the super-block.  The LDS slab is double-buffered, which
// makes the one barrier per super-block sufficient.  What a chunk's result is and how results combine is each kernel's own.
#pragma once

namespace kpr {

// V values of one column group
template <class T, int V>
struct ColVec {
    T v[V];
};

// the vector type that one access of a whole ColVec<T, V> goes through: float4 for float x 4 and float2 x 2, uint2 for unsigned x 2
// (its scalars are copied one by one below, as typed accesses: that is the code the kernels were tuned with)
template <class T> struct ColScalar { typedef T type; };
template <> struct ColScalar<float2> { typedef float type; };
template <class T, int V>
using ColWide = HIP_vector_type<typename ColScalar<T>::type, V * sizeof(T) / sizeof(typename ColScalar<T>::type)>;

// one access of V * sizeof(T) bytes (16 for float x 4 and float2 x 2), or one element
template <int V, class T>
KPR_DEV ColVec<T, V> col_load(const T* p) {
    ColVec<T, V> r;
    if constexpr (V > 1) {
        const ColWide<T, V> t = *reinterpret_cast<const ColWide<T, V>*>(p);
        auto* d = reinterpret_cast<typename ColScalar<T>::type*>(r.v);
#pragma unroll
        for (int i = 0; i < (int)(sizeof t / sizeof *d); ++i) d[i] = t[i];
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int V, class T>
KPR_DEV void col_store(T* p, const ColVec<T, V>& r) {
    if constexpr (V > 1) {
        ColWide<T, V> t;
        auto* s = reinterpret_cast<const typename ColScalar<T>::type*>(r.v);
#pragma unroll
        for (int i = 0; i < (int)(sizeof t / sizeof *s); ++i) t[i] = s[i];
        *reinterpret_cast<ColWide<T, V>*>(p) = t;
    } else {
        *p = r.v[0];
    }
}

// the column group of a lane: `item` is its outer item, `i0` its first inner index
struct ColGroup {
    int lane;
    long long group;
    bool live;
    long long item;
    unsigned i0;
};

template <int V>
KPR_DEV ColGroup col_group(long long n_groups, unsigned groups_per_item) {
    ColGroup g;
    g.lane = threadIdx.x & 63;
    g.group = (long long)blockIdx.x * 64 + g.lane;
    g.live = g.group < n_groups;
    // (a lane past the last group runs along on group 0 with its stores masked: the barrier needs every wave)
    const long long gsafe = g.live ? g.group : 0;
    g.item = gsafe / groups_per_item;
    g.i0 = (unsigned)(gsafe - g.item * groups_per_item) * V;
    return g;
}

}  // namespace kpr
