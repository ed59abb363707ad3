// Device steps the decoding selection kernels share (constrain.hip, beam.hip, decode.hip): the row log-sum-exp,
// the sorted-list top-K, the wave rank rounds and the row move.  Each is written once here, so two kernels that call one give the
// same bits for the same input -- the host replicas and the bit-exact tests rely on that.  A helper with a barrier, and a helper
// called between two barriers, is reached by every thread of the workgroup: a kernel's early returns come before its first call.
#pragma once
#include "common.h"

// ---- Row log-sum-exp of an fp32 row in a fixed order: a thread's chain, a fixed xor tree, the waves in order.  Two parts around the
// one barrier, which is the caller's: it may put reads of the raw row between them.

// The tree over a wave's 64 lanes, then lane 0's store of the wave's (mx, se) into rmx / rse[wave].
__device__ __forceinline__ void lse_wave_store(float& mx, float& se, float* rmx, float* rse) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(mx, se, __shfl_xor(mx, o, 64), __shfl_xor(se, o, 64));
    if ((threadIdx.x & 63) == 0) {
        rmx[threadIdx.x >> 6] = mx;
        rse[threadIdx.x >> 6] = se;
    }
}
// Part one, every thread of THREADS: thread t chains the 16-byte groups t, t + THREADS, ... of z[0 .. V & ~3), then the tail columns
// (V & ~3) + t, ...; then lse_wave_store.  z starts on 16 bytes (ld % 4 == 0 and an aligned base: the entry points' checks).
template <int THREADS>
__device__ __forceinline__ void row_lse_partials(const float* z, int V, float& mx, float& se, float* rmx, float* rse) {
    const int tid = threadIdx.x, vend = V & ~3;
    mx = -INFINITY;
    se = 0.f;
    for (int c4 = tid * 4; c4 < vend; c4 += THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(z + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) lse_add(mx, se, q[e]);
    }
    for (int c = vend + tid; c < V; c += THREADS) lse_add(mx, se, z[c]);
    lse_wave_store(mx, se, rmx, rse);
}
// a * b rounded to fp32 ON ITS OWN: the build contracts a plain product into the fma of whatever addition consumes it, and a value that
// is compared, listed and subtracted from in several places must be one number in all of them.  A constrained multiply is never fused.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp exceptions(strict)
    return a * b;
}
// Part one on the SCALED row v = mul_rounded(z, scale): the same columns, chain and tree.  At scale == 1.0f v is z, so the partials
// are row_lse_partials' bits.
template <int THREADS>
__device__ __forceinline__ void row_lse_partials_scaled(const float* z, int V, float scale, float& mx, float& se, float* rmx, float* rse) {
    const int tid = threadIdx.x, vend = V & ~3;
    mx = -INFINITY;
    se = 0.f;
    for (int c4 = tid * 4; c4 < vend; c4 += THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(z + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) lse_add(mx, se, mul_rounded(q[e], scale));
    }
    for (int c = vend + tid; c < V; c += THREADS) lse_add(mx, se, mul_rounded(z[c], scale));
    lse_wave_store(mx, se, rmx, rse);
}
// Part two, thread 0 after the barrier: its own wave's pair, then waves 1 .. THREADS / 64 - 1 in order.
template <int THREADS>
__device__ __forceinline__ float lse_waves_merge(float mx, float se, const float* rmx, const float* rse) {
    for (int k = 1; k < THREADS / 64; ++k) lse_merge(mx, se, rmx[k], rse[k]);
    return mx + logf(se);
}

// ---- Top-K of a workgroup's keys by sorted lists: every thread keeps its K best (key, index) pairs in MAXK registers, best first,
// and K rounds of a block arg-max over the list heads give the block's K best in order.
constexpr int TOPK_NONE = 0x7fffffff;                          // the index of an empty list slot (its key is -inf)
// (key descending, index ascending)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

template <int MAXK>
__device__ __forceinline__ void topk_clear(float (&kv)[MAXK], int (&ki)[MAXK]) {
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        kv[j] = -INFINITY;
        ki[j] = TOPK_NONE;
    }
}
// (cv, ci) into the first K slots by ripple: it takes the slot of the first pair it beats, which moves down one, and so on.
template <int MAXK>
__device__ __forceinline__ void topk_insert(float (&kv)[MAXK], int (&ki)[MAXK], int K, float cv, int ci) {
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        if (j < K && better(cv, ci, kv[j], ki[j])) {
            const float tv = kv[j];
            const int ti = ki[j];
            kv[j] = cv;
            ki[j] = ci;
            cv = tv;
            ci = ti;
        }
    }
}
template <int MAXK>
__device__ __forceinline__ void topk_pop(float (&kv)[MAXK], int (&ki)[MAXK]) {
#pragma unroll
    for (int t = 0; t < MAXK - 1; ++t) {
        kv[t] = kv[t + 1];
        ki[t] = ki[t + 1];
    }
    kv[MAXK - 1] = -INFINITY;
    ki[MAXK - 1] = TOPK_NONE;
}
// One round, three barriers: the best head of every wave by a fixed xor tree into sh_v / sh_i[wave]; thread 0 takes the waves in
// order, hands the winner to won(key, index) -- index TOPK_NONE: no list holds anything -- and broadcasts it through *sh_win; the
// thread whose head is the winner pops it (an index sits in one list only).
template <int THREADS, int MAXK, typename Won>
__device__ __forceinline__ void topk_round(float (&kv)[MAXK], int (&ki)[MAXK], float* sh_v, int* sh_i, int* sh_win, Won won) {
    const int tid = threadIdx.x;
    float bv = kv[0];
    int bi = ki[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if ((tid & 63) == 0) {
        sh_v[tid >> 6] = bv;
        sh_i[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < THREADS / 64; ++w)
            if (better(sh_v[w], sh_i[w], bv, bi)) {
                bv = sh_v[w];
                bi = sh_i[w];
            }
        won(bv, bi);
        *sh_win = bi;
    }
    __syncthreads();
    const int win = *sh_win;
    if (win != TOPK_NONE && ki[0] == win) topk_pop(kv, ki);
    __syncthreads();
}

// ---- Wave rank rounds: wave 0 of the workgroup ranks the K best of the WE keys in LDS (key descending, index ascending) into
// pick[0 .. K), TOPK_NONE where nothing is left; the other waves pass through.  taken[] is all 0 on entry and marks what was picked:
// lane l scans indices l, l + 64, ..., and the lane that scans the winner marks it itself, so no round needs a barrier.
__device__ __forceinline__ void wave_rank_rounds(const float* key, int* taken, int* pick, int WE, int K) {
    const int tid = threadIdx.x;
    if (tid >= 64) return;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = TOPK_NONE;
        for (int j = tid; j < WE; j += 64)
            if (!taken[j] && better(key[j], j, bv, bi)) {
                bv = key[j];
                bi = j;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (tid == 0) pick[k] = bi;
        if (bi != TOPK_NONE && (bi & 63) == tid) taken[bi] = 1;
    }
}

// ---- Row move: child row r0 + w of `rows` (W rows of ld elements from r0 on) becomes a copy of row par[w], columns [0, cols).  The
// parents are among the children's rows, so the invariant is: a thread reads column t of EVERY parent into registers before it
// writes column t of ANY child.  Columns are independent and each belongs to one thread, so no barrier is needed.
template <int MAXW, typename T>
__device__ __forceinline__ void move_rows(T* rows, int ld, const int* par, int r0, int W, int cols, int threads) {
    T v[MAXW];
    for (int t = threadIdx.x; t < cols; t += threads) {
#pragma unroll
        for (int w = 0; w < MAXW; ++w)
            if (w < W) v[w] = rows[(size_t)par[w] * ld + t];
#pragma unroll
        for (int w = 0; w < MAXW; ++w)
            if (w < W) rows[(size_t)(r0 + w) * ld + t] = v[w];
    }
}
