// The one bitonic network of the window data path (events.hip, finetune.hip).
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ int pow2_at_least(int v) {
    int n = 1;
    while (n < v) n <<= 1;
    return n;
}

// Ascending sort of n (a power of two) LDS positions by a whole workgroup of THREADS.  load(i) gives the entry at position i (anything
// with operator>), store(i, e) puts one there.  Both entries of a pair are read whole before they are compared: a "greater" and a
// "swap" on positions made the compiler read the pair sort's source indices twice, which the clock showed.  Equal entries only ever
// carry equal payloads here (padding, dropped events, equal frame values, or keys made unique by an index), so the result does not
// depend on how ties fall.
//
// One stage of the network: every aligned block of k2 positions that holds a bitonic sequence leaves sorted, ascending where
// (i & k2) == 0.  With k2 == n it is the final merge on its own: n positions that rise and then fall leave ascending (the merge
// passes of esim.hip load their second run reversed and call it alone).
template <int THREADS, class Load, class Store>
__device__ __forceinline__ void bitonic_stage_lds(int n, int k2, int tid, Load load, Store store) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < n; i += THREADS) {
            const int ixj = i ^ j;
            if (ixj > i) {
                const auto a = load(i), c = load(ixj);
                if ((a > c) == ((i & k2) == 0)) { store(i, c); store(ixj, a); }
            }
        }
        __syncthreads();
    }
}
template <int THREADS, class Load, class Store>
__device__ __forceinline__ void bitonic_sort_lds(int n, int tid, Load load, Store store) {
    for (int k2 = 2; k2 <= n; k2 <<= 1) bitonic_stage_lds<THREADS>(n, k2, tid, load, store);
}
template <int THREADS, class Key>
__device__ __forceinline__ void bitonic_sort_keys(Key* keys, int n, int tid) {
    bitonic_sort_lds<THREADS>(n, tid, [=](int i) { return keys[i]; }, [=](int i, Key k) { keys[i] = k; });
}
template <int THREADS, class Key>
__device__ __forceinline__ void bitonic_merge_keys(Key* keys, int n, int tid) {
    bitonic_stage_lds<THREADS>(n, n, tid, [=](int i) { return keys[i]; }, [=](int i, Key k) { keys[i] = k; });
}
