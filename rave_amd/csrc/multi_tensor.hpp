// What the multi-tensor elementwise kernels share (adam.hip, ema.hip): a table of tensors that travels BY VALUE in the kernel
// arguments (<= kMtItems tensors per launch), every workgroup takes kMtElems elements of ONE tensor and finds it by the prefix
// of workgroup counts.  A table type has `int blk_begin[kMtItems + 1]`, `int n[kMtItems]`, `int count` and its own pointers.
#pragma once
#include "common.hpp"

constexpr int kMtItems = 64;
constexpr int kMtElems = 2048;            // elements per workgroup (256 threads x 2 x 16 bytes)

// the table entry whose workgroups contain `block`
#define RH_MT_FIND(tb, lo)                                                           \
    int lo = 0, lo##_hi = (tb).count - 1;                                            \
    while (lo < lo##_hi) {                                                           \
        const int mid = (lo + lo##_hi + 1) >> 1;                                     \
        if ((tb).blk_begin[mid] <= (int)blockIdx.x) lo = mid; else lo##_hi = mid - 1; \
    }

// Host: fills `tb` from items[i ...] and returns its number of workgroups (0 = nothing left).  `i` is the consumed index: empty
// tensors are skipped without taking a table slot, so a chunk may span more than kMtItems items -- the next call continues
// where this one stopped (never re-processing an item).  put(tb, slot, item, index) stores the item's pointers.
template <typename Table, typename Item, typename Put>
inline int rh_mt_fill(Table& tb, const Item* items, int n_items, int& i, Put put) {
    int cnt = 0, blk = 0;
    for (; i < n_items && cnt < kMtItems; ++i) {
        const Item& it = items[i];
        if (it.n == 0) continue;
        put(tb, cnt, it, i);
        tb.n[cnt] = (int)it.n;
        tb.blk_begin[cnt] = blk;
        blk += (int)((it.n + kMtElems - 1) / kMtElems);
        ++cnt;
    }
    tb.blk_begin[cnt] = blk;
    tb.count = cnt;
    return blk;
}
