// Greedy-decode step kernels: everything position-dependent reads its position from DEVICE memory, so one captured
// hipGraph replays unchanged for every generated token (static KV cache, no host round trip per token).
#include "select_common.h"

namespace {

// x[b][:] = wte[ids[b][len-1]] + wpe[len-1+pos_offset]
__global__ __launch_bounds__(256) void embed_step_kernel(const int64_t* __restrict__ ids, int ids_ld,
                                                         const int* __restrict__ len_ptr, const float* __restrict__ wte,
                                                         const float* __restrict__ wpe, float* __restrict__ x, int d,
                                                         int pos_offset, int vocab) {
    const int b = blockIdx.x;
    const int t = *len_ptr - 1;
    long id = ids[(size_t)b * ids_ld + t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f32x4* e = reinterpret_cast<const f32x4*>(wte + (size_t)id * d);
    f32x4* o = reinterpret_cast<f32x4*>(x + (size_t)b * d);
    if (wpe) {
        const f32x4* p = reinterpret_cast<const f32x4*>(wpe + (size_t)(t + pos_offset) * d);
        for (int c = threadIdx.x; c < (d >> 2); c += 256) o[c] = e[c] + p[c];
    } else {
        for (int c = threadIdx.x; c < (d >> 2); c += 256) o[c] = e[c];
    }
}

// kcache[b][pos][:] = qkv[b][d:2d], vcache[b][pos][:] = qkv[b][2d:3d]
__global__ __launch_bounds__(256) void kv_append_kernel(const bf16_t* __restrict__ qkv, int qkv_rs, bf16_t* __restrict__ kc,
                                                        bf16_t* __restrict__ vc, long cache_bs, int cache_rs,
                                                        const int* __restrict__ pos_ptr, int d) {
    const int b = blockIdx.x, pos = *pos_ptr;
    const u32x4* src = reinterpret_cast<const u32x4*>(qkv + (size_t)b * qkv_rs + d);
    u32x4* kd = reinterpret_cast<u32x4*>(kc + (size_t)b * cache_bs + (size_t)pos * cache_rs);
    u32x4* vd = reinterpret_cast<u32x4*>(vc + (size_t)b * cache_bs + (size_t)pos * cache_rs);
    const int d8 = d >> 3;
    for (int c = threadIdx.x; c < d8; c += 256) {
        kd[c] = src[c];
        vd[c] = src[d8 + c];
    }
}

// One wave per (b, h).  Both passes over the cache use 16-byte loads with 8 lanes per key (lane = 8 * key_in_group + c,
// c = 16-byte chunk of the 64-wide head): one wave-instruction fetches 8 keys x 128 B = 8 full cache lines (the
// lane-per-key form issued 8 loads that each touched 64 lines).  Scores: per-lane partial dot over its 8 dims, 3 xor
// shuffles inside the 8-lane group.  Output: per-lane partial sum over its key stripe for its 8 dims, 3 xor shuffles
// across the 8 stripes.  The step is HBM-bound on the K/V cache (B x H x t x 256 B per call).
// append_dm > 0: q points at a packed [q | k | v] row of width 3*append_dm; the new token's k/v (this head's 64
// columns) are written into the cache at *pos by this workgroup and attended to from LDS (fused kv_append).
// HIST (beam search, i2t_beam_decode_attention): key t of row b is read from cache row hist[b][t] (hist null: row
// b / rows_per_mem for every key, the per-image cross-attention memory) through the LDS copy hs[] of the table row; the
// new token still lands in row b.  The table row is all that HIST changes -- same loads, same lanes, same reduction order:
// with an identity table the output is bit-equal.  HIST = false reads neither hs[] (no LDS for it) nor the last three arguments.
// The body is one device function, decode_attention_body: the kernel below hands it the key count n and `base`, the cache row its base
// pointers kb / vb address -- row b itself, or (HIST) row 0 -- and mem_decode_attention_kernel (i2t_mem_decode_attention: a memory
// stored once per image, row b over memory row mem_index[b]) the row its table names, with HIST = false and no append.
template <int WPB, bool HIST>         // waves (= heads) per workgroup: 49 152 one-wave workgroups per launch were dispatch-rate bound
__device__ __forceinline__ void decode_attention_body(const bf16_t* __restrict__ q, int q_rs, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                      long cache_bs, int cache_rs, long cache_hs, bf16_t* __restrict__ o, int o_rs, const int n,
                                                      int append_dm, const int* __restrict__ hist, int hist_ld, int rows_per_mem, const int base) {
    __shared__ float qs_[WPB][64], kn_[WPB][64], vn_[WPB][64];
    __shared__ float ps_[WPB][DECODE_MAX_KEYS];
    __shared__ int hs[HIST ? DECODE_MAX_KEYS : 1];
    const int wv = threadIdx.x >> 6;
    float* qs = qs_[wv];
    float* kn = kn_[wv];
    float* vn = vn_[wv];
    float* ps = ps_[wv];
    const int h = blockIdx.x * WPB + wv, b = blockIdx.y, lane = threadIdx.x & 63;
    const bf16_t* qrow = q + (size_t)b * q_rs + h * 64 + lane;
    qs[lane] = bf16_to_f32(qrow[0]);
    // the cache row kb / vb address is `base`: row b itself, or (HIST) row 0, where every key adds its own row and the new token adds `own`
    const int own = HIST ? b : 0;
    bf16_t* kb = kc + (size_t)base * cache_bs + (size_t)h * cache_hs;           // cache_hs = 64: token-major rows [t][H][64];
    bf16_t* vb = vc + (size_t)base * cache_bs + (size_t)h * cache_hs;           // cache_hs = tmax * 64 (cache_rs = 64): head-major [H][t][64]
    const int n_cached = append_dm > 0 ? n - 1 : n;          // keys read back from the cache
    if constexpr (HIST)
        for (int t = threadIdx.x; t < n_cached; t += 64 * WPB) hs[t] = hist ? hist[(size_t)b * hist_ld + t] : b / rows_per_mem;
    if (append_dm > 0) {
        const bf16_t kv = qrow[append_dm], vv = qrow[2 * append_dm];
        kn[lane] = bf16_to_f32(kv);
        vn[lane] = bf16_to_f32(vv);
        kb[(size_t)own * cache_bs + (size_t)(n - 1) * cache_rs + lane] = kv;
        vb[(size_t)own * cache_bs + (size_t)(n - 1) * cache_rs + lane] = vv;
    }
    __syncthreads();
    const int kg = lane >> 3, c = lane & 7;                  // key within a group of 8, 16-byte chunk of the head
    float qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = qs[c * 8 + e];
    float mx = -INFINITY;
    if (append_dm > 0 && lane == 0) {
        float s = 0.f;
        for (int e = 0; e < 64; ++e) s += kn[e] * qs[e];
        s *= 0.125f;
        ps[n - 1] = s;
        mx = s;
    }
    // 4 groups of 8 keys per trip: the four 16-byte loads are issued back to back (a one-group loop exposed the full HBM latency per
    // 8 keys: a caption's whole cache is 4-8 such groups, so the kernel ran latency-bound at 0.6 of the HBM roof)
    for (int k0 = 0; k0 < n_cached; k0 += 32) {
        u32x4 kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = k0 + 8 * u + kg;
            kk[u] = u32x4{0u, 0u, 0u, 0u};
            if (key < n_cached)
                kk[u] = *reinterpret_cast<const u32x4*>(kb + (size_t)key_row<HIST>(hs, key) * cache_bs + (size_t)key * cache_rs + c * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = k0 + 8 * u + kg;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += bf16lo(kk[u][e]) * qv[2 * e] + bf16hi(kk[u][e]) * qv[2 * e + 1];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            s *= 0.125f;
            if (key < n_cached) {
                if (c == 0) ps[key] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = wave_max(mx);
    __syncthreads();
    float sum = 0.f;
    for (int key = lane; key < n; key += 64) {
        float p = __expf(ps[key] - mx);
        ps[key] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int k0 = 0; k0 < n_cached; k0 += 32) {
        u32x4 vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = k0 + 8 * u + kg;
            vv[u] = u32x4{0u, 0u, 0u, 0u};
            if (key < n_cached)
                vv[u] = *reinterpret_cast<const u32x4*>(vb + (size_t)key_row<HIST>(hs, key) * cache_bs + (size_t)key * cache_rs + c * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = k0 + 8 * u + kg;
            const float p = key < n_cached ? ps[key] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += p * bf16lo(vv[u][e]);
                acc[2 * e + 1] += p * bf16hi(vv[u][e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {                            // sum the 8 key stripes (lanes with equal c)
        acc[e] += __shfl_xor(acc[e], 8, 64);
        acc[e] += __shfl_xor(acc[e], 16, 64);
        acc[e] += __shfl_xor(acc[e], 32, 64);
    }
    if (kg == 0) {
        const float inv = 1.0f / sum;
        if (append_dm > 0) {
            const float pn = ps[n - 1];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += pn * vn[c * 8 + e];
        }
        const u32x4 pk = {pack_bf16x2(acc[0] * inv, acc[1] * inv), pack_bf16x2(acc[2] * inv, acc[3] * inv),
                          pack_bf16x2(acc[4] * inv, acc[5] * inv), pack_bf16x2(acc[6] * inv, acc[7] * inv)};
        *reinterpret_cast<u32x4*>(o + (size_t)b * o_rs + h * 64 + c * 8) = pk;
    }
}

template <int WPB, bool HIST>
__global__ __launch_bounds__(64 * WPB) void decode_attention_kernel(const bf16_t* __restrict__ q, int q_rs,
                                                                    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                                    long cache_bs, int cache_rs, long cache_hs, bf16_t* __restrict__ o,
                                                                    int o_rs, const int* __restrict__ pos_ptr, int n_keys_fixed,
                                                                    int append_dm, const int* __restrict__ hist, int hist_ld,
                                                                    int rows_per_mem) {
    decode_attention_body<WPB, HIST>(q, q_rs, kc, vc, cache_bs, cache_rs, cache_hs, o, o_rs, pos_ptr ? (*pos_ptr + 1) : n_keys_fixed, append_dm,
                                     hist, hist_ld, rows_per_mem, HIST ? 0 : (int)blockIdx.y);
}

// i2t_mem_decode_attention: cross-attention of R rows over a memory stored once per image, [n_mem][n_keys][H 64] (token-major: heads 64
// apart, keys mem_rs apart).  Row b = blockIdx.y attends to the n_keys keys of memory row mem_index[b]: ONE wave-uniform word per
// workgroup, loaded once and folded into the base pointers -- no table in LDS, nothing per key (the HIST form fills hs[t] = b /
// rows_per_mem for every key and reads it back per load).  Everything else is decode_attention_body<WPB, false> without append: the
// same loads, lanes and reduction order, so the output is bit-equal to decode_attention_kernel<WPB, false> on the gathered memory.
// The values of mem_index are NOT checked here: the host validates them (0 <= mem_index[r] < n_mem) before it uploads the table.
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void mem_decode_attention_kernel(const bf16_t* __restrict__ q, int q_rs, const bf16_t* __restrict__ kmem,
                                                                        const bf16_t* __restrict__ vmem, long mem_bs, int mem_rs,
                                                                        bf16_t* __restrict__ o, int o_rs, int n_keys,
                                                                        const int* __restrict__ mem_index) {
    decode_attention_body<WPB, false>(q, q_rs, const_cast<bf16_t*>(kmem), const_cast<bf16_t*>(vmem), mem_bs, mem_rs, 64, o, o_rs, n_keys, 0,
                                      nullptr, 0, 1, mem_index[blockIdx.y]);
}

// HF NoRepeatNGramLogitsProcessor + argmax for one caption per workgroup.  A row with no finite allowed column (all banned)
// gets token 0, torch.argmax's answer for a row of -inf, and margin 0.
constexpr int BAN_THREADS = 1024;
// LP (i2t_ngram_ban_argmax_lp, a caption step): the same choice, and tok_lp[b][len] = z[chosen] - logsumexp(z[b][:V]) over the RAW
// row -- the ban does not enter -- from an online (max, sum exp) pass folded into the scan: per thread in its scan order, then
// select_common.h's lse_wave_store and lse_waves_merge at 1024 threads.  Nothing is written once *done is set.
template <bool F32, bool LP>
__global__ __launch_bounds__(BAN_THREADS) void ngram_ban_argmax_kernel(const void* __restrict__ logits, int ld,
                                                                       int64_t* __restrict__ ids, int ids_ld,
                                                                       const int* __restrict__ len_ptr,
                                                                       const int* __restrict__ ngram_sizes, int n_sizes,
                                                                       int V, float* __restrict__ margin_out,
                                                                       const int* __restrict__ done, float* __restrict__ tok_lp, int lp_ld) {
    extern __shared__ unsigned dyn_lds[];              // ban bitmap, ceil(V / 32) words
    __shared__ float rv[BAN_THREADS / 64], rv2[BAN_THREADS / 64];
    __shared__ int ri[BAN_THREADS / 64];
    __shared__ float rmx[LP ? BAN_THREADS / 64 : 1], rse[LP ? BAN_THREADS / 64 : 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (LP)
        if (*done) return;                              // block-uniform, before any barrier
    const int len = *len_ptr;
    int64_t* row = ids + (size_t)b * ids_ld;
    unsigned* banbits = dyn_lds;
    build_ban_bitmap(banbits, row, len, ngram_sizes, n_sizes, V, BAN_THREADS);
    float best = -INFINITY, second = -INFINITY;
    int bi = 0x7fffffff;
    float mx = -INFINITY, se = 0.f;                     // (LP) the raw row's online softmax pair
    // fp32 rows with ld % 4 == 0 (the decode path pads to 8): 16-byte loads, 4 consecutive columns per lane per step
    // (the scalar scan ran at ~2.3 TB/s).  Per lane the columns are still visited in ascending order: first index wins ties.
    const bool vec4 = F32 && (ld & 3) == 0 && ((uintptr_t)logits & 15) == 0;
    const int vend = vec4 ? (V & ~3) : 0;
    for (int c4 = tid * 4; c4 < vend; c4 += BAN_THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(logits) + (size_t)b * ld + c4);
        const unsigned nib = (banbits[c4 >> 5] >> (c4 & 31)) & 15u;     // c4 % 4 == 0: the 4 columns' bits share a word
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = ((nib >> e) & 1u) ? -INFINITY : q[e];
            const int c = c4 + e;
            if constexpr (LP) lse_add(mx, se, q[e]);
            if (v > best) {
                second = best;
                best = v;
                bi = c;
            } else if (v > second) {
                second = v;
            }
        }
    }
    for (int c = vend + tid; c < V; c += BAN_THREADS) {
        float v = F32 ? reinterpret_cast<const float*>(logits)[(size_t)b * ld + c]
                      : bf16_to_f32(reinterpret_cast<const bf16_t*>(logits)[(size_t)b * ld + c]);
        if constexpr (LP) lse_add(mx, se, v);
        if (ban_bit(banbits, c)) v = -INFINITY;
        if (v > best) {                                   // strided ascending scan: first index wins ties
            second = best;
            best = v;
            bi = c;
        } else if (v > second) {
            second = v;
        }
    }
    // wave reduce (value desc, index asc), tracking the runner-up for the margin
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(best, o, 64), os = __shfl_xor(second, o, 64);
        int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) {
            second = fmaxf(best, os);
            best = ov;
            bi = oi;
        } else {
            second = fmaxf(second, ov);
        }
    }
    const int w = tid >> 6;
    if constexpr (LP) lse_wave_store(mx, se, rmx, rse);
    if ((tid & 63) == 0) {
        rv[w] = best;
        rv2[w] = second;
        ri[w] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < BAN_THREADS / 64; ++k) {
            if (rv[k] > best || (rv[k] == best && ri[k] < bi)) {
                second = fmaxf(best, rv2[k]);
                best = rv[k];
                bi = ri[k];
            } else {
                second = fmaxf(second, rv[k]);
            }
        }
        const bool none = bi == 0x7fffffff;                  // every column banned or -inf
        row[len] = none ? 0 : bi;
        if (margin_out) margin_out[b] = none ? 0.f : best - second;
        if constexpr (LP) {
            const int tok = none ? 0 : bi;
            const float z = F32 ? reinterpret_cast<const float*>(logits)[(size_t)b * ld + tok]
                                : bf16_to_f32(reinterpret_cast<const bf16_t*>(logits)[(size_t)b * ld + tok]);
            tok_lp[(size_t)b * lp_ld + len] = z - lse_waves_merge<BAN_THREADS>(mx, se, rmx, rse);
        }
    }
}

// The same token choice from the lm_head's SEGMENT maxima (i2t_gemm_bf16_top2: the two largest logits of every 64-column segment of a
// row, value descending / column ascending) instead of the logits themselves: a segment whose best column is not banned contributes
// it, one whose best is banned contributes its second, and one whose two best are BOTH banned (rare: two continuations of repeated
// n-grams among 64 neighbouring token ids, both ahead of everything else there) is re-evaluated exactly here -- 64 dot products of
// the hidden row with the head's rows, banned columns left out.  Such segments are marked in an LDS bitmap of ceil(nseg / 32) words
// behind the ban bitmap, so however many there are, none is dropped; each wave re-evaluates the marked segments of every fourth word.
// One caption per workgroup; a row with every column banned gets token 0.
// LP (i2t_top2_ngram_argmax_lp, a caption step after i2t_gemm_bf16_top2_lse): the same choice, and tok_lp[b][len] = z[chosen] - lse with
// lse from the segments' (v1, se) pairs -- one wave, lane l merges segments l, l + 64, ... in ascending order, then a fixed xor tree, as
// lse_token_logprob_kernel below -- and z[chosen] re-evaluated in fp32 from the bf16 operands (the chosen column may be token 0 of a
// row with everything banned, of which the segments hold nothing).  The ban does not enter the lse.  Nothing is written once *done is set.
constexpr int T2_THREADS = 256;
template <bool LP>
__global__ __launch_bounds__(T2_THREADS) void top2_ngram_argmax_kernel(const f32x4* __restrict__ top2, int nseg, const bf16_t* __restrict__ hid,
                                                                        int ld_h, const bf16_t* __restrict__ W, int ldw, int d,
                                                                        int64_t* __restrict__ ids, int ids_ld, const int* __restrict__ len_ptr,
                                                                        const int* __restrict__ ngram_sizes, int n_sizes, int V,
                                                                        const float* __restrict__ seg_se, const int* __restrict__ done,
                                                                        float* __restrict__ tok_lp, int lp_ld) {
    extern __shared__ unsigned dyn_lds[];              // ban bitmap (ceil(V / 32) words), then the redo bitmap (ceil(nseg / 32) words)
    __shared__ float rv[T2_THREADS / 64];
    __shared__ int ri[T2_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (LP)
        if (*done) return;                              // block-uniform, before any barrier
    const int len = *len_ptr;
    int64_t* row = ids + (size_t)b * ids_ld;
    unsigned* banbits = dyn_lds;
    unsigned* redo = dyn_lds + (V + 31) / 32;
    const int nrw = (nseg + 31) / 32;
    for (int w = tid; w < nrw; w += T2_THREADS) redo[w] = 0u;
    build_ban_bitmap(banbits, row, len, ngram_sizes, n_sizes, V, T2_THREADS);      // (its barriers also cover the redo clear)
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto offer = [&](float v, int c) {
        if (v > best || (v == best && c < bi)) {
            best = v;
            bi = c;
        }
    };
    for (int sgm = tid; sgm < nseg; sgm += T2_THREADS) {
        const f32x4 t = top2[(size_t)b * nseg + sgm];
        const int i1 = __float_as_int(t[1]), i2 = __float_as_int(t[3]);
        if (!(t[0] > -INFINITY)) continue;                  // nothing valid in the segment
        if ((unsigned)i1 >= (unsigned)V) continue;          // (a column index outside the vocabulary: never from i2t_gemm_bf16_top2)
        if (!ban_bit(banbits, i1)) {
            offer(t[0], i1);
        } else if (t[2] > -INFINITY && (unsigned)i2 < (unsigned)V && !ban_bit(banbits, i2)) {
            offer(t[2], i2);
        } else if (t[2] > -INFINITY) {                      // both leaders banned: what is left of the segment is unknown
            atomicOr(&redo[sgm >> 5], 1u << (sgm & 31));
        }
    }
    __syncthreads();
    for (int w = wave; w < nrw; w += T2_THREADS / 64) {     // exact re-evaluation of a segment, one column per lane of the wave
        unsigned m = redo[w];
        while (m) {                                          // wave-uniform
            const int sgm = w * 32 + __builtin_ctz(m);
            m &= m - 1u;
            const int c = sgm * 64 + lane;
            if (c < V && !ban_bit(banbits, c)) {
                const bf16_t* wr = W + (size_t)c * ldw;
                const bf16_t* hr = hid + (size_t)b * ld_h;
                float acc = 0.f;
                for (int k = 0; k < d; k += 8) {
                    const u32x4 wv = *reinterpret_cast<const u32x4*>(wr + k), hv = *reinterpret_cast<const u32x4*>(hr + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc += bf16lo(wv[e]) * bf16lo(hv[e]) + bf16hi(wv[e]) * bf16hi(hv[e]);
                }
                offer(acc, c);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        offer(ov, oi);
    }
    if (lane == 0) {
        rv[wave] = best;
        ri[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < T2_THREADS / 64; ++k) offer(rv[k], ri[k]);
        row[len] = bi == 0x7fffffff ? 0 : bi;               // every column banned or -inf: torch.argmax's 0
        if constexpr (LP) ri[0] = bi == 0x7fffffff ? 0 : bi;
    }
    if constexpr (LP) {
        __syncthreads();
        if (wave != 0) return;
        const int tok = ri[0];
        float mx = -INFINITY, se = 0.f;
        for (int sgm = lane; sgm < nseg; sgm += 64) lse_merge(mx, se, top2[(size_t)b * nseg + sgm][0], seg_se[(size_t)b * nseg + sgm]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lse_merge(mx, se, __shfl_xor(mx, o, 64), __shfl_xor(se, o, 64));
        const bf16_t* wr = W + (size_t)tok * ldw;
        const bf16_t* hr = hid + (size_t)b * ld_h;
        float z = 0.f;
        for (int k = 8 * lane; k < d; k += 8 * 64) {
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wr + k), hv = *reinterpret_cast<const u32x4*>(hr + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) z += bf16lo(wv[e]) * bf16lo(hv[e]) + bf16hi(wv[e]) * bf16hi(hv[e]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) tok_lp[(size_t)b * lp_ld + len] = z - (mx + logf(se));
    }
}

// Caption scoring: log p(label | row) from the lm_head's SEGMENT statistics (i2t_gemm_bf16_lse: (max, sum exp) of every 64-column
// segment of a row of scale . hidden . W^T).  One wave per row: lane l merges segments l, l + 64, ... in ascending order, the 64
// partial pairs are merged by a fixed xor tree (no atomics: bit-reproducible), lse = mx + log(se); the label's own logit is
// re-evaluated here in fp32 from the bf16 operands (as top2_ngram_argmax_kernel re-evaluates a segment), so the GEMM needs no labels.
constexpr int LSE_WAVES = 4;
__global__ __launch_bounds__(64 * LSE_WAVES) void lse_token_logprob_kernel(const float* __restrict__ stats, int nseg, const bf16_t* __restrict__ hid,
                                                                           int ld_h, const bf16_t* __restrict__ W, int ldw, int d, float scale,
                                                                           const int64_t* __restrict__ labels, int64_t ignore_index,
                                                                           float* __restrict__ lse, float* __restrict__ logprob, int M, int V) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * LSE_WAVES + (threadIdx.x >> 6);
    if (m >= M) return;                                      // wave-uniform
    const f32x2* row = reinterpret_cast<const f32x2*>(stats) + (size_t)m * nseg;
    float mx = -INFINITY, se = 0.f;
    for (int sgm = lane; sgm < nseg; sgm += 64) {
        const f32x2 t = row[sgm];
        lse_merge(mx, se, t[0], t[1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(mx, se, __shfl_xor(mx, o, 64), __shfl_xor(se, o, 64));
    const float l = mx + logf(se);
    const int64_t lab = labels[m];
    const bool live = lab != ignore_index && lab >= 0 && lab < (int64_t)V;      // wave-uniform
    float z = 0.f;
    if (live) {
        const bf16_t* wr = W + (size_t)lab * ldw;
        const bf16_t* hr = hid + (size_t)m * ld_h;
        for (int k = 8 * lane; k < d; k += 8 * 64) {
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wr + k), hv = *reinterpret_cast<const u32x4*>(hr + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) z += bf16lo(wv[e]) * bf16lo(hv[e]) + bf16hi(wv[e]) * bf16hi(hv[e]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
    }
    if (lane == 0) {
        lse[m] = l;
        logprob[m] = live ? scale * z - l : 0.f;
    }
}

// The finish rule of a caption step, after the step's token landed at ids[r][len]: a row that finished earlier gets the
// pad id and log-prob 0 there; a row whose new token is EOS is finished, its length len + 1 (the EOS kept).  ctrl[1] = rows still
// unfinished (i2t_beam_advance raises ctrl[0] when it is 0); without an EOS id the equal-length form keeps it at R.
// RAGGED: rows whose prompts differ in length.  Row r of image b = r / N is forced to its prompt while len < plen[b]
// (whatever the chooser wrote there is replaced, log-prob 0, the row counts as unfinished) and emits from plen[b] on, where the rule
// above holds and the max_new-th emitted token finishes the row as well.  A column outside the id / log-prob rows is not touched
// (ctrl[1] then stays 0 and i2t_beam_advance ends the steps).  The equal-length form reads neither prompt nor plen (both null).
// One workgroup, block reduction, no atomics.
constexpr int FIN_THREADS = 1024;
template <bool RAGGED>
__global__ __launch_bounds__(FIN_THREADS) void caption_finish_kernel(int64_t* __restrict__ ids, int ids_ld, const int* __restrict__ len_ptr,
                                                                     const int64_t* __restrict__ prompt, int prompt_ld,
                                                                     const int* __restrict__ plen, int N, int max_new, int eos, int64_t pad,
                                                                     int* __restrict__ finished, int* __restrict__ lengths,
                                                                     float* __restrict__ tok_lp, int lp_ld, int* __restrict__ ctrl, int R) {
    __shared__ int red[FIN_THREADS / 64];
    if (ctrl[0]) return;                                 // block-uniform: no thread writes ctrl[0]
    const int len = *len_ptr, tid = threadIdx.x;
    if constexpr (RAGGED) {
        if (len < 0 || len >= ids_ld || len >= lp_ld) return;
    }
    int live = 0;
    for (int r = tid; r < R; r += FIN_THREADS) {
        int64_t* id = ids + (size_t)r * ids_ld + len;
        float* lp = tok_lp + (size_t)r * lp_ld + len;
        int b = 0, p = 0;
        bool forced = false, spent = false;
        if constexpr (RAGGED) {
            b = r / N;
            p = plen[b];
            forced = len < p && len < prompt_ld;
            spent = len + 1 - p >= max_new;
        }
        if (forced) {
            *id = prompt[(size_t)b * prompt_ld + len];
            *lp = 0.f;
            ++live;
        } else if (finished[r]) {
            *id = pad;
            *lp = 0.f;
        } else if ((eos >= 0 && *id == (int64_t)eos) || spent) {
            finished[r] = 1;
            lengths[r] = len + 1;
        } else {
            ++live;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = live;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int k = 0; k < FIN_THREADS / 64; ++k) t += red[k];
        ctrl[1] = !RAGGED && eos < 0 ? R : t;
    }
}

// The logits processors of a caption step, a pre-pass over the step's fp32 logits row before the chooser: repetition
// penalty over ids[r][0 .. len), suppressed ids, EOS below the minimum length -- transformers' RepetitionPenalty -> SuppressTokens ->
// MinNewTokensLength order.  One workgroup per row.  Pass A: the RAW row's log-sum-exp (select_common.h's row_lse_partials /
// lse_waves_merge: bit-reproducible, the bits i2t_rows_lse gives for the row) -> raw_lse[r].  Pass B: saved[r][j] = z[ids[r][j]], all raw
// since nothing has been written.  Barrier.  Pass C: z[ids[r][j]] = f(saved[r][j]); every occurrence of a token reads the same raw
// value and stores the same result, so a token is penalised once however often it occurs, with no first-occurrence search.  Barrier.
// Pass D: the suppress list and the min-length EOS, plain stores of -inf that read nothing.  An id outside [0, V) takes no part
// (saved 0).  Nothing is read or written once *done is set.  decoding.process_logits_host is the host's statement of passes C and D.
constexpr int PROC_THREADS = 256;
__global__ __launch_bounds__(PROC_THREADS) void caption_logits_process_kernel(float* logits, int ld, const int64_t* __restrict__ ids, int ids_ld,
                                                                              const int* __restrict__ len_ptr, const int* __restrict__ plen,
                                                                              int P, int N, const int* __restrict__ suppress, int n_suppress,
                                                                              int eos, int min_new, float theta, float inv_theta,
                                                                              const int* __restrict__ done, float* __restrict__ raw_lse,
                                                                              float* saved, int saved_ld, int V) {
    __shared__ float rmx[PROC_THREADS / 64], rse[PROC_THREADS / 64];
    if (*done) return;                                  // block-uniform, before any barrier
    const int r = blockIdx.x, tid = threadIdx.x;
    int len = *len_ptr;
    len = len < 0 ? 0 : (len > ids_ld ? ids_ld : len);
    float* z = logits + (size_t)r * ld;
    const int64_t* row = ids + (size_t)r * ids_ld;
    float* sv = saved + (size_t)r * saved_ld;
    float mx, se;
    row_lse_partials<PROC_THREADS>(z, V, mx, se, rmx, rse);
    for (int j = tid; j < len; j += PROC_THREADS) {
        const int64_t t = row[j];
        sv[j] = (t >= 0 && t < V) ? z[t] : 0.f;
    }
    __syncthreads();                                    // every read of the raw row is done
    if (tid == 0) raw_lse[r] = lse_waves_merge<PROC_THREADS>(mx, se, rmx, rse);
    for (int j = tid; j < len; j += PROC_THREADS) {
        const int64_t t = row[j];
        if (t >= 0 && t < V) {
            const float v = sv[j];                      // this thread's own store of pass B
            z[t] = v > 0.f ? v * inv_theta : v * theta;
        }
    }
    __syncthreads();
    for (int i = tid; i < n_suppress; i += PROC_THREADS) {
        const int t = suppress[i];
        if (t >= 0 && t < V) z[t] = -INFINITY;
    }
    if (tid == 0 && eos >= 0) {
        const int p = plen ? plen[r / N] : P;
        if (len - p < min_new) z[eos] = -INFINITY;
    }
}

// After the chooser of a processed step: tok_lp[r][len] = z_raw[c] - raw_lse[r] for the chosen c = ids[r][len], over the chooser's
// value (which it took on the processed row).  The raw z[c] is saved[r][j] for any j < len with ids[r][j] == c (they all hold the same
// value; the largest such j is taken), else logits[r][c], which pass C never wrote; a suppressed or min-length-banned token is not
// chosen, so pass D needs no restore.  One wave per row, nothing is written once *done is set.
constexpr int RAWLP_WAVES = 4;
__global__ __launch_bounds__(64 * RAWLP_WAVES) void caption_raw_logprob_kernel(const int64_t* __restrict__ ids, int ids_ld,
                                                                               const int* __restrict__ len_ptr, const float* __restrict__ raw_lse,
                                                                               const float* __restrict__ saved, int saved_ld,
                                                                               const float* __restrict__ logits, int ld, const int* __restrict__ done,
                                                                               float* __restrict__ tok_lp, int lp_ld, int R, int V) {
    if (*done) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * RAWLP_WAVES + (threadIdx.x >> 6);
    const int len = *len_ptr;
    if (r >= R || len < 0 || len >= ids_ld || len >= lp_ld) return;      // wave-uniform
    const int64_t* row = ids + (size_t)r * ids_ld;
    const int64_t c = row[len];
    if (c < 0 || c >= V) return;                        // (never from a chooser)
    int at = -1;
    for (int j = lane; j < len; j += 64)
        if (row[j] == c) at = j;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) at = max(at, __shfl_xor(at, o, 64));
    if (lane == 0) {
        const float zc = at >= 0 ? saved[(size_t)r * saved_ld + at] : logits[(size_t)r * ld + c];
        tok_lp[(size_t)r * lp_ld + len] = zc - raw_lse[r];
    }
}

// The alternatives of a caption step (generate_captions' top_logprobs), right behind the lm_head GEMM and before anything
// writes the row: for column len = *len_ptr of row r, the K best columns of the RAW fp32 row by (z descending, id ascending), their
// log-probs z - lse(z), and the row's entropy -sum p log p.  One workgroup per row at rows_lse_kernel's thread count, two passes over the
// row (the second an L2 read).  Pass A: select_common.h's row_lse_partials / lse_waves_merge -- the bits i2t_rows_lse gives for the row --,
// broadcast through LDS.  Pass B, each thread over the same columns in the same order: the entropy term p (lse - z), p = exp(z - lse)
// (a -inf column has p = 0 and adds nothing), and the thread's K best in a sorted register list (topk_insert), a candidate first held
// against the list's last live slot: a thread sees V / 256 columns and almost none enter.  Then K topk_round's give the row's K best in
// order, thread 0 storing each as it is found; the entropy goes a thread's chain -> a fixed xor tree -> the waves in order.  No atomics:
// two launches give the same bits.  Nothing is read or written once *done is set, for a finished row, for a row whose column is still
// inside its prompt (plen, int32 [R / N], or null: no row is) or for a column outside the outputs; else exactly column len of the row's
// three outputs is written.  Columns [V, ld) are never read.  decoding_host.top_logprobs_host is the host's statement.
constexpr int TOPLP_THREADS = 256;                      // = TRIE_THREADS of constrain.hip's rows_lse_kernel: the lse's bits depend on it
constexpr int TOPLP_MAXK = 8;
__global__ __launch_bounds__(TOPLP_THREADS) void caption_top_logprobs_kernel(const float* __restrict__ logits, int ld, const int* __restrict__ len_ptr,
                                                                             const int* __restrict__ plen, int N, const int* __restrict__ finished,
                                                                             const int* __restrict__ done, int* __restrict__ top_tok,
                                                                             float* __restrict__ top_lp, float* __restrict__ entropy, int out_ld,
                                                                             int K, int V) {
    constexpr int WAVES = TOPLP_THREADS / 64;
    __shared__ float rmx[WAVES], rse[WAVES], sh_v[WAVES], sh_h[WAVES], sh_lse;
    __shared__ int sh_i[WAVES], sh_win;
    if (*done) return;                                  // block-uniform, as every return before the first barrier
    const int r = blockIdx.x, tid = threadIdx.x, len = *len_ptr;
    if (len < 0 || len >= out_ld || finished[r]) return;
    if (plen && len < plen[r / N]) return;              // a forced column
    const float* z = logits + (size_t)r * ld;
    float mx, se;
    row_lse_partials<TOPLP_THREADS>(z, V, mx, se, rmx, rse);
    __syncthreads();
    if (tid == 0) sh_lse = lse_waves_merge<TOPLP_THREADS>(mx, se, rmx, rse);
    __syncthreads();
    const float lse = sh_lse;
    float kv[TOPLP_MAXK], lastv = -INFINITY, h = 0.f;
    int ki[TOPLP_MAXK], lasti = TOPK_NONE;              // (lastv, lasti): a copy of list slot K - 1, so no register is indexed by K
    topk_clear(kv, ki);
    auto offer = [&](float v, int c) {
        if (v > -INFINITY) {
            const float dlt = lse - v;
            h += __expf(-dlt) * dlt;
        }
        if (better(v, c, lastv, lasti)) {
            topk_insert(kv, ki, K, v, c);
#pragma unroll
            for (int j = 0; j < TOPLP_MAXK; ++j)
                if (j == K - 1) {
                    lastv = kv[j];
                    lasti = ki[j];
                }
        }
    };
    const int vend = V & ~3;                            // (ld % 4 == 0 and a 16-byte base: the entry point's checks)
    for (int c4 = tid * 4; c4 < vend; c4 += TOPLP_THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(z + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) offer(q[e], c4 + e);
    }
    for (int c = vend + tid; c < V; c += TOPLP_THREADS) offer(z[c], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    if ((tid & 63) == 0) sh_h[tid >> 6] = h;            // read by thread 0 behind the rounds' barriers (K >= 1)
    const size_t cell = (size_t)r * out_ld + len;
#pragma unroll 1
    for (int j = 0; j < K; ++j)
        topk_round<TOPLP_THREADS>(kv, ki, sh_v, sh_i, &sh_win, [&](float bv, int bi) {
            top_tok[cell * K + j] = bi == TOPK_NONE ? -1 : bi;      // (K <= V: every round finds a column)
            top_lp[cell * K + j] = bv - lse;
        });
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) h += sh_h[w];
        entropy[cell] = h;
    }
}

// The same for a caption that is GIVEN (VisionEncoderDecoder.score's top_logprobs), behind the fp32 lm_head GEMM of a chunk
// of teacher-forced rows: for every row r, on v = z * scale (mul_rounded: one fp32 rounding per column, the same number wherever it is
// used), the K best columns by (v descending, id ascending), their log-probs v - lse(v), the entropy, the row's lse, and for the row's
// label y the log-prob v_y - lse and the RANK: the number of columns strictly ahead of y in that order.  The kernel above with the
// label's two outputs added and no step state: one workgroup per row, pass A the shared fixed-order lse on the scaled row (at scale 1
// the bits i2t_rows_lse gives), pass B over the same columns in the same order with the entropy term, the thread's sorted K-list and an
// integer count of better(v_c, c, v_y, y) -- v_y is loaded once before the pass; integer sums are order-free --, then K topk_round's
// and thread 0's stores.  The list entry at the label's rank and the label's log-prob are the same subtraction on the same two numbers:
// the same bits.  A label that is ignore_index or outside [0, V) gives rank -1 and logprob 0 and counts nothing; every row gets the
// other outputs.  No atomics.  Columns [V, ld) are never read.  decoding_host.score_top_logprobs_host is the host's statement.
__global__ __launch_bounds__(TOPLP_THREADS) void score_top_logprobs_kernel(const float* __restrict__ logits, int ld, float scale,
                                                                           const int64_t* __restrict__ labels, int64_t ignore_index,
                                                                           int* __restrict__ top_tok, float* __restrict__ top_lp,
                                                                           float* __restrict__ entropy, int* __restrict__ rank,
                                                                           float* __restrict__ lse_out, float* __restrict__ logprob, int K, int V) {
    constexpr int WAVES = TOPLP_THREADS / 64;
    __shared__ float rmx[WAVES], rse[WAVES], sh_v[WAVES], sh_h[WAVES], sh_lse;
    __shared__ int sh_i[WAVES], sh_n[WAVES], sh_win;
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (size_t)r * ld;
    const int64_t lab = labels[r];
    const bool live = lab != ignore_index && lab >= 0 && lab < V;       // block-uniform
    const int y = live ? (int)lab : 0;
    const float vy = live ? mul_rounded(z[y], scale) : 0.f;
    float mx, se;
    row_lse_partials_scaled<TOPLP_THREADS>(z, V, scale, mx, se, rmx, rse);
    __syncthreads();
    if (tid == 0) sh_lse = lse_waves_merge<TOPLP_THREADS>(mx, se, rmx, rse);
    __syncthreads();
    const float lse = sh_lse;
    float kv[TOPLP_MAXK], lastv = -INFINITY, h = 0.f;
    int ki[TOPLP_MAXK], lasti = TOPK_NONE, ahead = 0;   // (lastv, lasti): a copy of list slot K - 1, so no register is indexed by K
    topk_clear(kv, ki);
    auto offer = [&](float zc, int c) {
        const float v = mul_rounded(zc, scale);
        if (v > -INFINITY) {
            const float dlt = lse - v;
            h += __expf(-dlt) * dlt;
        }
        ahead += live && better(v, c, vy, y);
        if (better(v, c, lastv, lasti)) {
            topk_insert(kv, ki, K, v, c);
#pragma unroll
            for (int j = 0; j < TOPLP_MAXK; ++j)
                if (j == K - 1) {
                    lastv = kv[j];
                    lasti = ki[j];
                }
        }
    };
    const int vend = V & ~3;                            // (ld % 4 == 0 and a 16-byte base: the entry point's checks)
    for (int c4 = tid * 4; c4 < vend; c4 += TOPLP_THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(z + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) offer(q[e], c4 + e);
    }
    for (int c = vend + tid; c < V; c += TOPLP_THREADS) offer(z[c], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        h += __shfl_xor(h, o, 64);
        ahead += __shfl_xor(ahead, o, 64);
    }
    if ((tid & 63) == 0) {                              // read by thread 0 behind the rounds' barriers (K >= 1)
        sh_h[tid >> 6] = h;
        sh_n[tid >> 6] = ahead;
    }
#pragma unroll 1
    for (int j = 0; j < K; ++j)
        topk_round<TOPLP_THREADS>(kv, ki, sh_v, sh_i, &sh_win, [&](float bv, int bi) {
            top_tok[(size_t)r * K + j] = bi == TOPK_NONE ? -1 : bi;     // (K <= V: every round finds a column)
            top_lp[(size_t)r * K + j] = bv - lse;
        });
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) {
            h += sh_h[w];
            ahead += sh_n[w];
        }
        entropy[r] = h;
        lse_out[r] = lse;
        rank[r] = live ? ahead : -1;
        logprob[r] = live ? vy - lse : 0.f;
    }
}

__global__ void advance_kernel(int* counters, int n, int delta) {
    if ((int)threadIdx.x < n) counters[threadIdx.x] += delta;
}

// Prompt prefill: the K and V rows a forward pass saved for m tokens of B images go to cache slots slot0 .. slot0 + m - 1 of the N
// cache rows b * N .. b * N + N - 1 of every image.  One thread per 16-byte chunk of a source row's K (and the chunk of its V at the
// same column): chunk index fastest, so a wave reads 1 KB runs of a source row, and its stores go out as groups of hd / 8 lanes
// that each fill one head's hd * 2 bytes of a cache slot -- 8 lanes x 16 B = one whole 128-byte line in the head-major layout
// [R][H][clen][64], where (head, slot) rows are exactly one line; in the row-major layout [R][clen][w] the wave's stores are one
// contiguous run of the slot's row.  The two chunks are loaded once and stored N times: nothing else depends on N.
// Element (row r, head h, slot s, column c) of a cache is at r * cache_bs + h * cache_hs + s * cache_rs + c, as
// decode_attention_kernel (kb / vb) and gq_decode_attention address it.
__global__ __launch_bounds__(256) void kv_prefill_kernel(const bf16_t* __restrict__ src, int src_ld, int k_off, int v_off, int src_T,
                                                         int src_t0, int m, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, long cache_bs,
                                                         int cache_rs, long cache_hs, int hd, int w8, int slot0, long total, int N) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % w8);                          // 16-byte chunk of the w = 8 * w8 K (or V) columns
    const long bt = idx / w8;
    const int t = (int)(bt % m);
    const long b = bt / m;
    const int col = ch * 8, h = col / hd, c = col - h * hd;
    const bf16_t* s = src + (size_t)(b * src_T + src_t0 + t) * src_ld + col;
    const u32x4 kk = *reinterpret_cast<const u32x4*>(s + k_off);
    const u32x4 vv = *reinterpret_cast<const u32x4*>(s + v_off);
    const size_t at = (size_t)(b * N) * cache_bs + (size_t)h * cache_hs + (size_t)(slot0 + t) * cache_rs + c;
    for (int n = 0; n < N; ++n) {
        *reinterpret_cast<u32x4*>(kc + at + (size_t)n * cache_bs) = kk;
        *reinterpret_cast<u32x4*>(vc + at + (size_t)n * cache_bs) = vv;
    }
}

}  // namespace

extern "C" int i2t_embed_step(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const float* wte,
                              const float* wpe, float* x, int B, int d, int pos_offset, int vocab) {
    I2T_REQUIRE(ids && len_ptr && wte && x && B > 0 && d % 4 == 0, "i2t_embed_step: bad args");
    hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, ids_ld, len_ptr, wte, wpe, x, d,
                       pos_offset, vocab);
    I2T_CHECK_LAUNCH("i2t_embed_step");
    return I2T_OK;
}

extern "C" int i2t_kv_append(void* stream, const void* qkv, int qkv_rs, void* kcache, void* vcache, long cache_bs,
                             int cache_rs, const int* pos_ptr, int B, int d) {
    I2T_REQUIRE(qkv && kcache && vcache && pos_ptr && B > 0 && d % 8 == 0 && qkv_rs % 8 == 0 && cache_rs % 8 == 0 &&
                    cache_bs % 8 == 0,
                "i2t_kv_append: bad args");
    hipLaunchKernelGGL(kv_append_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, qkv_rs,
                       (bf16_t*)kcache, (bf16_t*)vcache, cache_bs, cache_rs, pos_ptr, d);
    I2T_CHECK_LAUNCH("i2t_kv_append");
    return I2T_OK;
}

extern "C" int i2t_kv_prefill(void* stream, const void* src, int src_ld, int k_off, int v_off, int src_T, int src_t0, int m, void* kcache,
                              void* vcache, long cache_bs, int cache_rs, long cache_hs, int hd, int w, int slot0, int B, int N) {
    I2T_REQUIRE(src && kcache && vcache, "i2t_kv_prefill: null pointer");
    I2T_REQUIRE(w > 0 && w % 8 == 0, "i2t_kv_prefill: w = %d: the K / V width must be a positive multiple of 8", w);
    I2T_REQUIRE(hd > 0 && hd % 8 == 0 && w % hd == 0, "i2t_kv_prefill: hd = %d: the head width must be a multiple of 8 that divides w = %d", hd, w);
    I2T_REQUIRE(src_ld > 0 && src_ld % 8 == 0, "i2t_kv_prefill: src_ld = %d: source rows must be a multiple of 8 elements apart", src_ld);
    I2T_REQUIRE(k_off >= 0 && v_off >= 0 && k_off % 8 == 0 && v_off % 8 == 0 && k_off + w <= src_ld && v_off + w <= src_ld,
                "i2t_kv_prefill: k_off = %d, v_off = %d: column offsets must be multiples of 8 with w = %d columns inside src_ld = %d", k_off,
                v_off, w, src_ld);
    I2T_REQUIRE(ALIGNED16(src) && ALIGNED16(kcache) && ALIGNED16(vcache), "i2t_kv_prefill: misaligned base pointer (16 bytes)");
    I2T_REQUIRE(cache_bs > 0 && cache_rs > 0 && cache_hs > 0 && cache_bs % 8 == 0 && cache_rs % 8 == 0 && cache_hs % 8 == 0,
                "i2t_kv_prefill: cache strides (%ld, %d, %ld) must be positive multiples of 8", cache_bs, cache_rs, cache_hs);
    I2T_REQUIRE(B >= 1 && N >= 1, "i2t_kv_prefill: B = %d images, N = %d rows per image", B, N);
    I2T_REQUIRE(m >= 1, "i2t_kv_prefill: m = %d: at least one token", m);
    I2T_REQUIRE(src_t0 >= 0 && (long)src_t0 + m <= src_T, "i2t_kv_prefill: src_t0 + m = %d + %d exceeds src_T = %d", src_t0, m, src_T);
    const long Hkv = w / hd, end = (long)slot0 + m;
    // row-major [R][clen][w]: heads are hd apart inside a slot's row; head-major [R][Hkv][clen][hd-wide rows]: slots inside a head's run
    const bool row_major = cache_hs == hd && cache_rs >= w;
    const bool fits = row_major ? end * cache_rs <= cache_bs : (cache_rs >= hd && end * cache_rs <= cache_hs && Hkv * cache_hs <= cache_bs);
    I2T_REQUIRE(slot0 >= 0 && fits, "i2t_kv_prefill: slot0 + m = %d + %d exceeds the slots a cache row holds (strides %ld, %d, %ld)", slot0, m,
                cache_bs, cache_rs, cache_hs);
    const int w8 = w / 8;
    const long total = (long)B * m * w8, blocks = (total + 255) / 256;
    I2T_REQUIRE(blocks <= 0x7fffffffL, "i2t_kv_prefill: %ld chunks exceed one grid", total);
    hipLaunchKernelGGL(kv_prefill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, src_ld, k_off, v_off,
                       src_T, src_t0, m, (bf16_t*)kcache, (bf16_t*)vcache, cache_bs, cache_rs, cache_hs, hd, w8, slot0, total, N);
    I2T_CHECK_LAUNCH("i2t_kv_prefill");
    return I2T_OK;
}

// i2t_decode_attention and i2t_beam_decode_attention (fn: the entry point the messages name): one set of checks, one launch
static int decode_attention(const char* fn, bool beam, void* stream, const void* q, int q_rs, void* kcache, void* vcache, long cache_bs,
                            int cache_rs, long cache_hs, void* o, int o_rs, const int* pos_ptr, int n_keys_fixed, int append_dm,
                            const int* hist, int hist_ld, int rows_per_mem, int B, int H) {
    I2T_REQUIRE(cache_hs >= 64 && cache_hs % 8 == 0, "%s: head stride %ld", fn, cache_hs);
    I2T_REQUIRE(append_dm == 0 || (pos_ptr && append_dm == 64 * H), "%s: append needs pos_ptr and a packed qkv row", fn);
    I2T_REQUIRE(q && kcache && vcache && o && B > 0 && H > 0 && (!beam || rows_per_mem >= 1), "%s: bad args", fn);
    I2T_REQUIRE(pos_ptr || (n_keys_fixed > 0 && n_keys_fixed <= DECODE_MAX_KEYS), "%s: key count out of range", fn);
    I2T_REQUIRE(!beam || !hist || hist_ld >= (pos_ptr ? 1 : n_keys_fixed), "%s: history rows shorter than the keys", fn);
    I2T_REQUIRE(cache_rs % 8 == 0 && cache_bs % 8 == 0 && ALIGNED16(kcache) && ALIGNED16(vcache), "%s: cache misaligned", fn);
    I2T_REQUIRE(o_rs % 8 == 0 && ALIGNED16(o), "%s: output rows must be 16-byte aligned", fn);
    const bool w4 = H % 4 == 0;
    const auto kernel = w4 ? (beam ? decode_attention_kernel<4, true> : decode_attention_kernel<4, false>)
                           : (beam ? decode_attention_kernel<1, true> : decode_attention_kernel<1, false>);
    hipLaunchKernelGGL(kernel, w4 ? dim3(H / 4, B) : dim3(H, B), dim3(w4 ? 256 : 64), 0, (hipStream_t)stream, (const bf16_t*)q, q_rs,
                       (bf16_t*)kcache, (bf16_t*)vcache, cache_bs, cache_rs, cache_hs, (bf16_t*)o, o_rs, pos_ptr, n_keys_fixed, append_dm,
                       hist, hist_ld, rows_per_mem);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

extern "C" int i2t_decode_attention(void* stream, const void* q, int q_rs, void* kcache, void* vcache,
                                    long cache_bs, int cache_rs, long cache_hs, void* o, int o_rs, const int* pos_ptr, int n_keys_fixed,
                                    int append_dm, int B, int H) {
    return decode_attention("i2t_decode_attention", false, stream, q, q_rs, kcache, vcache, cache_bs, cache_rs, cache_hs, o, o_rs, pos_ptr,
                            n_keys_fixed, append_dm, nullptr, 0, 1, B, H);
}

extern "C" int i2t_beam_decode_attention(void* stream, const void* q, int q_rs, void* kcache, void* vcache, long cache_bs, int cache_rs,
                                         long cache_hs, void* o, int o_rs, const int* pos_ptr, int n_keys_fixed, int append_dm,
                                         const int* hist, int hist_ld, int rows_per_mem, int R, int H) {
    return decode_attention("i2t_beam_decode_attention", true, stream, q, q_rs, kcache, vcache, cache_bs, cache_rs, cache_hs, o, o_rs,
                            pos_ptr, n_keys_fixed, append_dm, hist, hist_ld, rows_per_mem, R, H);
}

// Cross-attention of R rows over a memory stored once per image: row r attends to the n_keys keys of memory row mem_index[r] (head h
// of memory row m starts at kmem + m * mem_bs + h * 64, its keys mem_rs apart).  No append, no position, no history table.  The
// VALUES of mem_index are the caller's to check -- 0 <= mem_index[r] < n_mem, validated on the host before the table is uploaded --:
// the kernel does not scan them, and n_mem is here for the checks below only.
extern "C" int i2t_mem_decode_attention(void* stream, const void* q, int q_rs, const void* kmem, const void* vmem, long mem_bs, int mem_rs,
                                        void* o, int o_rs, int n_keys, const int* mem_index, int n_mem, int R, int H) {
    const char* fn = "i2t_mem_decode_attention";
    I2T_REQUIRE(q && kmem && vmem && o, "%s: null operand", fn);
    I2T_REQUIRE(mem_index, "%s: mem_index is required (one memory row per query row)", fn);
    I2T_REQUIRE(R > 0 && H > 0, "%s: R = %d rows, H = %d heads", fn, R, H);
    I2T_REQUIRE(n_keys >= 1 && n_keys <= DECODE_MAX_KEYS, "%s: n_keys = %d: key count out of range (1 .. %d)", fn, n_keys, DECODE_MAX_KEYS);
    I2T_REQUIRE(n_mem >= 1, "%s: n_mem = %d: at least one memory row", fn, n_mem);
    I2T_REQUIRE(mem_rs >= 64 * H && mem_rs % 8 == 0 && mem_bs >= (long)n_keys * mem_rs && mem_bs % 8 == 0 && ALIGNED16(kmem) && ALIGNED16(vmem),
                "%s: memory misaligned or rows too short (mem_bs = %ld, mem_rs = %d for %d keys of %d heads of 64)", fn, mem_bs, mem_rs, n_keys, H);
    I2T_REQUIRE(q_rs >= 64 * H && o_rs >= 64 * H && o_rs % 8 == 0 && ALIGNED16(o), "%s: output rows must be 16-byte aligned and hold H * 64 columns", fn);
    const bool w4 = H % 4 == 0;
    hipLaunchKernelGGL(w4 ? mem_decode_attention_kernel<4> : mem_decode_attention_kernel<1>, w4 ? dim3(H / 4, R) : dim3(H, R),
                       dim3(w4 ? 256 : 64), 0, (hipStream_t)stream, (const bf16_t*)q, q_rs, (const bf16_t*)kmem, (const bf16_t*)vmem, mem_bs, mem_rs,
                       (bf16_t*)o, o_rs, n_keys, mem_index);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

extern "C" int i2t_ngram_ban_argmax(void* stream, const void* logits, int ld, int logits_is_f32, int64_t* ids, int ids_ld,
                                    int* len_ptr, const int* ngram_sizes, int n_sizes, int B, int V, float* margin_out) {
    I2T_REQUIRE(logits && ids && len_ptr && B > 0 && V > 0 && (n_sizes == 0 || ngram_sizes), "i2t_ngram_ban_argmax: bad args");
    const size_t lds = (size_t)(V + 31) / 32 * sizeof(unsigned);
    I2T_REQUIRE(lds <= BAN_LDS_MAX, "i2t_ngram_ban_argmax: vocabulary %d: the ban bitmap exceeds %d bytes of LDS", V, BAN_LDS_MAX);
    if (logits_is_f32)
        hipLaunchKernelGGL((ngram_ban_argmax_kernel<true, false>), dim3(B), dim3(BAN_THREADS), lds, (hipStream_t)stream, logits, ld, ids,
                           ids_ld, len_ptr, ngram_sizes, n_sizes, V, margin_out, nullptr, nullptr, 0);
    else
        hipLaunchKernelGGL((ngram_ban_argmax_kernel<false, false>), dim3(B), dim3(BAN_THREADS), lds, (hipStream_t)stream, logits, ld, ids,
                           ids_ld, len_ptr, ngram_sizes, n_sizes, V, margin_out, nullptr, nullptr, 0);
    I2T_CHECK_LAUNCH("i2t_ngram_ban_argmax");
    return I2T_OK;
}

extern "C" int i2t_ngram_ban_argmax_lp(void* stream, const float* logits, int ld, int64_t* ids, int ids_ld, const int* len_ptr,
                                       const int* ngram_sizes, int n_sizes, int B, int V, const int* done, float* tok_lp, int lp_ld) {
    I2T_REQUIRE(logits && ids && len_ptr && done && tok_lp && B > 0 && V > 0 && ld >= V && (n_sizes == 0 || ngram_sizes),
                "i2t_ngram_ban_argmax_lp: bad args");
    const size_t lds = (size_t)(V + 31) / 32 * sizeof(unsigned);
    I2T_REQUIRE(lds <= BAN_LDS_MAX, "i2t_ngram_ban_argmax_lp: vocabulary %d: the ban bitmap exceeds %d bytes of LDS", V, BAN_LDS_MAX);
    hipLaunchKernelGGL((ngram_ban_argmax_kernel<true, true>), dim3(B), dim3(BAN_THREADS), lds, (hipStream_t)stream, logits, ld, ids, ids_ld,
                       len_ptr, ngram_sizes, n_sizes, V, nullptr, done, tok_lp, lp_ld);
    I2T_CHECK_LAUNCH("i2t_ngram_ban_argmax_lp");
    return I2T_OK;
}

extern "C" int i2t_top2_ngram_argmax(void* stream, const float* top2, int nseg, const void* hidden, int ld_hidden, const void* w_head,
                                     int ld_w, int d, int64_t* ids, int ids_ld, int* len_ptr, const int* ngram_sizes, int n_sizes, int B, int V) {
    I2T_REQUIRE(top2 && hidden && w_head && ids && len_ptr && B > 0 && V > 0 && nseg == (V + 63) / 64 && (n_sizes == 0 || ngram_sizes),
                "i2t_top2_ngram_argmax: bad args (nseg must be ceil(V / 64))");
    I2T_REQUIRE(d % 8 == 0 && (ld_hidden & 7) == 0 && (ld_w & 7) == 0 && ALIGNED16(top2) && ALIGNED16(hidden) && ALIGNED16(w_head),
                "i2t_top2_ngram_argmax: hidden / head rows must be 16-byte aligned, d %% 8 == 0");
    const size_t lds = ((size_t)(V + 31) / 32 + (nseg + 31) / 32) * sizeof(unsigned);
    I2T_REQUIRE(lds <= BAN_LDS_MAX, "i2t_top2_ngram_argmax: vocabulary %d: the ban bitmaps exceed %d bytes of LDS", V, BAN_LDS_MAX);
    hipLaunchKernelGGL(top2_ngram_argmax_kernel<false>, dim3(B), dim3(T2_THREADS), lds, (hipStream_t)stream, (const f32x4*)top2, nseg,
                       (const bf16_t*)hidden, ld_hidden, (const bf16_t*)w_head, ld_w, d, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, V,
                       nullptr, nullptr, nullptr, 0);
    I2T_CHECK_LAUNCH("i2t_top2_ngram_argmax");
    return I2T_OK;
}

extern "C" int i2t_top2_ngram_argmax_lp(void* stream, const float* top2, const float* se, int nseg, const void* hidden, int ld_hidden,
                                        const void* w_head, int ld_w, int d, int64_t* ids, int ids_ld, const int* len_ptr, const int* ngram_sizes,
                                        int n_sizes, int B, int V, const int* done, float* tok_lp, int lp_ld) {
    I2T_REQUIRE(top2 && se && hidden && w_head && ids && len_ptr && done && tok_lp && B > 0 && V > 0 && nseg == (V + 63) / 64 &&
                    (n_sizes == 0 || ngram_sizes),
                "i2t_top2_ngram_argmax_lp: bad args (nseg must be ceil(V / 64))");
    I2T_REQUIRE(d > 0 && d % 8 == 0 && (ld_hidden & 7) == 0 && (ld_w & 7) == 0 && ld_hidden >= d && ld_w >= d && ALIGNED16(top2) &&
                    ALIGNED16(hidden) && ALIGNED16(w_head),
                "i2t_top2_ngram_argmax_lp: hidden / head rows must be 16-byte aligned, d %% 8 == 0");
    const size_t lds = ((size_t)(V + 31) / 32 + (nseg + 31) / 32) * sizeof(unsigned);
    I2T_REQUIRE(lds <= BAN_LDS_MAX, "i2t_top2_ngram_argmax_lp: vocabulary %d: the ban bitmaps exceed %d bytes of LDS", V, BAN_LDS_MAX);
    hipLaunchKernelGGL(top2_ngram_argmax_kernel<true>, dim3(B), dim3(T2_THREADS), lds, (hipStream_t)stream, (const f32x4*)top2, nseg,
                       (const bf16_t*)hidden, ld_hidden, (const bf16_t*)w_head, ld_w, d, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, V, se, done,
                       tok_lp, lp_ld);
    I2T_CHECK_LAUNCH("i2t_top2_ngram_argmax_lp");
    return I2T_OK;
}

extern "C" int i2t_caption_finish(void* stream, int64_t* ids, int ids_ld, const int* len_ptr, int eos, int64_t pad, int* finished, int* lengths,
                                  float* tok_lp, int lp_ld, int* ctrl, int R) {
    I2T_REQUIRE(ids && len_ptr && finished && lengths && tok_lp && ctrl && R > 0 && ids_ld > 0 && lp_ld > 0, "i2t_caption_finish: bad args");
    hipLaunchKernelGGL(caption_finish_kernel<false>, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, ids, ids_ld, len_ptr,
                       (const int64_t*)nullptr, 0, (const int*)nullptr, 1, 0, eos, pad, finished, lengths, tok_lp, lp_ld, ctrl, R);
    I2T_CHECK_LAUNCH("i2t_caption_finish");
    return I2T_OK;
}

extern "C" int i2t_caption_finish_ragged(void* stream, int64_t* ids, int ids_ld, const int* len_ptr, const int64_t* prompt, int prompt_ld,
                                         const int* plen, int N, int max_new, int eos, int64_t pad, int* finished, int* lengths, float* tok_lp,
                                         int lp_ld, int* ctrl, int R) {
    I2T_REQUIRE(ids && len_ptr && prompt && plen && finished && lengths && tok_lp && ctrl && R > 0 && ids_ld > 0 && lp_ld > 0 && prompt_ld > 0,
                "i2t_caption_finish_ragged: bad args");
    I2T_REQUIRE(N >= 1 && R % N == 0 && max_new >= 1, "i2t_caption_finish_ragged: %d rows in groups of %d, max_new %d", R, N, max_new);
    hipLaunchKernelGGL(caption_finish_kernel<true>, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, ids, ids_ld, len_ptr, prompt, prompt_ld,
                       plen, N, max_new, eos, pad, finished, lengths, tok_lp, lp_ld, ctrl, R);
    I2T_CHECK_LAUNCH("i2t_caption_finish_ragged");
    return I2T_OK;
}

extern "C" int i2t_caption_logits_process(void* stream, float* logits, int ld, const int64_t* ids, int ids_ld, const int* len_ptr, const int* plen,
                                          int P, int N, const int* suppress, int n_suppress, int eos, int min_new, float theta, float inv_theta,
                                          const int* done, float* raw_lse, float* saved, int saved_ld, int R, int V) {
    I2T_REQUIRE(logits && ids && len_ptr && done && raw_lse && saved, "i2t_caption_logits_process: null pointer");
    I2T_REQUIRE(n_suppress == 0 || suppress, "i2t_caption_logits_process: n_suppress = %d without a list", n_suppress);
    I2T_REQUIRE(R > 0 && V > 0 && ids_ld > 0, "i2t_caption_logits_process: R = %d rows, V = %d, ids_ld = %d", R, V, ids_ld);
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "i2t_caption_logits_process: ld = %d: logits rows hold V = %d columns and start on 16 bytes", ld, V);
    I2T_REQUIRE(saved_ld >= ids_ld, "i2t_caption_logits_process: saved_ld = %d is shorter than the id rows (ids_ld = %d)", saved_ld, ids_ld);
    I2T_REQUIRE(n_suppress >= 0 && n_suppress < V, "i2t_caption_logits_process: n_suppress = %d: between 0 and V - 1 = %d ids", n_suppress, V - 1);
    I2T_REQUIRE(eos < V, "i2t_caption_logits_process: eos = %d outside the vocabulary of %d", eos, V);
    I2T_REQUIRE(min_new >= 0, "i2t_caption_logits_process: min_new = %d", min_new);
    I2T_REQUIRE(theta > 0.f && inv_theta > 0.f && theta < INFINITY && inv_theta < INFINITY,
                "i2t_caption_logits_process: theta = %g, 1 / theta = %g: both positive and finite", (double)theta, (double)inv_theta);
    I2T_REQUIRE(N >= 1 && R % N == 0 && P >= 0, "i2t_caption_logits_process: %d rows in groups of %d, P = %d", R, N, P);
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(saved) && ALIGNED16(raw_lse) && ALIGNED16(ids),
                "i2t_caption_logits_process: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(caption_logits_process_kernel, dim3(R), dim3(PROC_THREADS), 0, (hipStream_t)stream, logits, ld, ids, ids_ld, len_ptr, plen,
                       P, N, suppress, n_suppress, eos, min_new, theta, inv_theta, done, raw_lse, saved, saved_ld, V);
    I2T_CHECK_LAUNCH("i2t_caption_logits_process");
    return I2T_OK;
}

extern "C" int i2t_caption_raw_logprob(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const float* raw_lse, const float* saved,
                                       int saved_ld, const float* logits, int ld, const int* done, float* tok_lp, int lp_ld, int R, int V) {
    I2T_REQUIRE(ids && len_ptr && raw_lse && saved && logits && done && tok_lp, "i2t_caption_raw_logprob: null pointer");
    I2T_REQUIRE(R > 0 && V > 0 && ids_ld > 0 && lp_ld > 0, "i2t_caption_raw_logprob: R = %d rows, V = %d, ids_ld = %d, lp_ld = %d", R, V, ids_ld,
                lp_ld);
    I2T_REQUIRE(ld >= V, "i2t_caption_raw_logprob: ld = %d: logits rows hold V = %d columns", ld, V);
    I2T_REQUIRE(saved_ld >= ids_ld, "i2t_caption_raw_logprob: saved_ld = %d is shorter than the id rows (ids_ld = %d)", saved_ld, ids_ld);
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(saved) && ALIGNED16(raw_lse) && ALIGNED16(ids),
                "i2t_caption_raw_logprob: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(caption_raw_logprob_kernel, dim3((R + RAWLP_WAVES - 1) / RAWLP_WAVES), dim3(64 * RAWLP_WAVES), 0, (hipStream_t)stream, ids,
                       ids_ld, len_ptr, raw_lse, saved, saved_ld, logits, ld, done, tok_lp, lp_ld, R, V);
    I2T_CHECK_LAUNCH("i2t_caption_raw_logprob");
    return I2T_OK;
}

extern "C" int i2t_caption_top_logprobs(void* stream, const float* logits, int ld, const int* len_ptr, const int* plen, int N,
                                        const int* finished, const int* done, int* top_tok, float* top_lp, float* entropy, int out_ld, int K,
                                        int R, int V) {
    I2T_REQUIRE(logits && len_ptr && finished && done && top_tok && top_lp && entropy, "i2t_caption_top_logprobs: null pointer");
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "i2t_caption_top_logprobs: ld = %d: logits rows hold V = %d columns and start on 16 bytes", ld, V);
    I2T_REQUIRE(ALIGNED16(logits), "i2t_caption_top_logprobs: misaligned base pointer (16 bytes)");
    I2T_REQUIRE(K >= 1 && K <= TOPLP_MAXK, "i2t_caption_top_logprobs: K = %d: from 1 to %d alternatives", K, TOPLP_MAXK);
    I2T_REQUIRE(K <= V, "i2t_caption_top_logprobs: K = %d alternatives of a vocabulary of %d", K, V);
    I2T_REQUIRE(out_ld > 0 && N > 0 && R > 0, "i2t_caption_top_logprobs: out_ld = %d, N = %d, R = %d: all positive", out_ld, N, R);
    hipLaunchKernelGGL(caption_top_logprobs_kernel, dim3(R), dim3(TOPLP_THREADS), 0, (hipStream_t)stream, logits, ld, len_ptr, plen, N, finished,
                       done, top_tok, top_lp, entropy, out_ld, K, V);
    I2T_CHECK_LAUNCH("i2t_caption_top_logprobs");
    return I2T_OK;
}

extern "C" int i2t_score_top_logprobs(void* stream, const float* logits, int ld, float scale, const int64_t* labels, int64_t ignore_index,
                                      int* top_tok, float* top_lp, float* entropy, int* rank, float* lse, float* logprob, int K, int R, int V) {
    I2T_REQUIRE(logits && labels && top_tok && top_lp && entropy && rank && lse && logprob, "i2t_score_top_logprobs: null pointer");
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "i2t_score_top_logprobs: ld = %d: logits rows hold V = %d columns and start on 16 bytes", ld, V);
    I2T_REQUIRE(ALIGNED16(logits), "i2t_score_top_logprobs: misaligned base pointer (16 bytes)");
    I2T_REQUIRE(K >= 1 && K <= TOPLP_MAXK, "i2t_score_top_logprobs: K = %d: from 1 to %d alternatives", K, TOPLP_MAXK);
    I2T_REQUIRE(K <= V, "i2t_score_top_logprobs: K = %d alternatives of a vocabulary of %d", K, V);
    I2T_REQUIRE(R > 0, "i2t_score_top_logprobs: R = %d rows", R);
    I2T_REQUIRE(scale > 0.f && scale < INFINITY, "i2t_score_top_logprobs: scale = %g: finite and positive", (double)scale);
    hipLaunchKernelGGL(score_top_logprobs_kernel, dim3(R), dim3(TOPLP_THREADS), 0, (hipStream_t)stream, logits, ld, scale, labels, ignore_index,
                       top_tok, top_lp, entropy, rank, lse, logprob, K, V);
    I2T_CHECK_LAUNCH("i2t_score_top_logprobs");
    return I2T_OK;
}

extern "C" int i2t_lse_token_logprob(void* stream, const float* stats, int nseg, const void* hidden, int ld_hidden, const void* w_head, int ld_w,
                                     int d, float scale, const int64_t* labels, int64_t ignore_index, float* lse, float* logprob, int M, int V) {
    I2T_REQUIRE(stats && hidden && w_head && labels && lse && logprob && M > 0 && V > 0 && d > 0 && nseg == (V + 63) / 64,
                "i2t_lse_token_logprob: bad args (nseg must be ceil(V / 64))");
    I2T_REQUIRE(d % 8 == 0 && (ld_hidden & 7) == 0 && (ld_w & 7) == 0 && ld_hidden >= d && ld_w >= d && ALIGNED16(hidden) && ALIGNED16(w_head) &&
                    (((uintptr_t)stats) & 7) == 0,
                "i2t_lse_token_logprob: hidden / head rows must be 16-byte aligned, d %% 8 == 0, stats 8-byte aligned");
    hipLaunchKernelGGL(lse_token_logprob_kernel, dim3((M + LSE_WAVES - 1) / LSE_WAVES), dim3(64 * LSE_WAVES), 0, (hipStream_t)stream, stats, nseg,
                       (const bf16_t*)hidden, ld_hidden, (const bf16_t*)w_head, ld_w, d, scale, labels, ignore_index, lse, logprob, M, V);
    I2T_CHECK_LAUNCH("i2t_lse_token_logprob");
    return I2T_OK;
}

extern "C" int i2t_advance(void* stream, int* counters, int n, int delta) {
    I2T_REQUIRE(counters && n > 0 && n <= 64, "i2t_advance: bad args");
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, n, delta);
    I2T_CHECK_LAUNCH("i2t_advance");
    return I2T_OK;
}
