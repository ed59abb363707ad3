// Beam-search step kernels over the static KV cache (reference models/generation_utils.py:10-148, BeamSearchTokenGenerator).
// R = B * W rows, batch-major (row r = b * W + w).  Every position-dependent input (pos, len, the "all beams ended" flag) lives in
// device memory, so one captured hipGraph replays the whole step once per token with no host round trip:
//   decoder blocks (the HIST attention kernels of decode.hip / family.hip) -> lm_head (fp32 logits) -> i2t_beam_candidates -> i2t_beam_consolidate -> i2t_beam_advance.
// Survivors never copy K/V: a history table hist[R][T] (int32) names the physical cache row that holds key t of beam r.  The step
// writes its new K/V at physical (r, pos); consolidation sets hist[child][t] = hist[parent][t] for t < pos and hist[child][pos] =
// parent.  Each position of each physical row is written once, so no entry a live beam points at is ever overwritten.  A sparse
// layer caches its kept positions only (slot = rank among them): key s of beam r is at (hist[r][slot_pos[s]], s), and a slot
// written again before a kept token lands there is named by no history.
#include "common.h"

namespace {

__device__ __forceinline__ unsigned bmix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// counter-based uniform in (0, 1) on a grid of 2^-23, a pure function of (seed, step, row, index, salt); image2text_amd/rng.py::beam_uniform
// is the host replica.  salt 0: candidate draws (row = beam row, index = token id); salt 1: consolidation (row = caption, index =
// flat candidate w * E + e).
__device__ __forceinline__ float beam_uniform(const unsigned* seed, unsigned step, unsigned row, unsigned index, unsigned salt) {
    const unsigned h1 = bmix32(seed[0] ^ (row * 0x9E3779B9u));
    const unsigned h2 = bmix32(h1 + seed[1] + step * 0x85EBCA6Bu + salt * 0x27D4EB2Fu);
    const unsigned h = bmix32(h2 + index * 0x165667B1u);
    return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);     // exact in fp32: 23 bits + 1/2
}
// Gumbel noise: key = logit + gumbel; the top-k keys are k draws without replacement, in draw order, from softmax(logits)
__device__ __forceinline__ float gumbel(float u) { return -logf(-logf(u)); }

__device__ __forceinline__ unsigned okey(float f) {            // monotone float -> unsigned (no NaNs on this path)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// (value descending, index ascending)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

constexpr int BC_THREADS = 1024, BC_MAX_E = 16;

// One workgroup per beam row.  The row is streamed from the logits (fp32, 16-byte loads, every lane visits its columns in
// ascending order): the top-k threshold by bisection on the order-preserving integer image of the scores (only with a crop, 32
// block-wide counts), then ONE pass that keeps the online max / sum of exp of the scores and a per-lane list of the E best keys
// (raw score or score / T + Gumbel noise), merged across the block in E rounds.
__global__ __launch_bounds__(BC_THREADS) void beam_candidates_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ ids,
                                                                     int ids_ld, const int* __restrict__ len_ptr, const int* __restrict__ done,
                                                                     const int* __restrict__ ngram_sizes, int n_sizes, int V, int E,
                                                                     float temperature, int top_k, int eos, float log_boost,
                                                                     const unsigned* __restrict__ seed, int* __restrict__ cand_tok,
                                                                     float* __restrict__ cand_lp, int* __restrict__ raw_tok) {
    extern __shared__ unsigned dyn_lds[];                  // ban bitmap, ceil(V / 32) words
    __shared__ float redf[BC_THREADS / 64];
    __shared__ int redi[BC_THREADS / 64];
    __shared__ float sh_v[BC_THREADS / 64];
    __shared__ int sh_i[BC_THREADS / 64];
    __shared__ int sel[BC_MAX_E];
    if (*done) return;                                     // every beam has ended: the replays that are left do nothing
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = *len_ptr;
    const int64_t* row = ids + (size_t)r * ids_ld;
    const float* src = logits + (size_t)r * ld;
    unsigned* banbits = dyn_lds;
    build_ban_bitmap(banbits, row, len, ngram_sizes, n_sizes, V, BC_THREADS);
    auto score = [&](int c, float v) { return ban_bit(banbits, c) ? -INFINITY : v; };

    // ---- top-k: key of the k-th largest score (everything below it is cropped; ties at the threshold stay)
    unsigned kth = 0u;
    if (top_k > 0 && top_k < V) {
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = kth | (1u << bit);
            int cnt = 0;
            for (int c4 = tid * 4; c4 < V; c4 += BC_THREADS * 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(src + c4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c4 + e < V) cnt += okey(score(c4 + e, q[e])) >= cand ? 1 : 0;
            }
            float t = block_sum((float)cnt, redf);          // exact: counts <= V < 2^24
            if ((int)t >= top_k) kth = cand;
        }
    }
    const bool sampled = temperature > 0.f;

    // ---- one pass: online logsumexp of y = score (/ T) over the kept set, per-lane top-E of the keys
    float m = -INFINITY, z = 0.f;
    float kv[BC_MAX_E];
    int ki[BC_MAX_E];
#pragma unroll
    for (int j = 0; j < BC_MAX_E; ++j) { kv[j] = -INFINITY; ki[j] = 0x7fffffff; }
    float last = -INFINITY;                                 // the list's E-th key
    for (int c4 = tid * 4; c4 < V; c4 += BC_THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(src + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c4 + e;
            if (c >= V) break;
            float s = score(c, q[e]);
            if (okey(s) < kth) s = -INFINITY;
            if (s == -INFINITY) continue;
            const float y = sampled ? s / temperature : s;
            if (y > m) {
                z = z * __expf(m - y) + 1.f;
                m = y;
            } else {
                z += __expf(y - m);
            }
            const float key = sampled ? y + gumbel(beam_uniform(seed, (unsigned)len, (unsigned)r, (unsigned)c, 0u)) : y;
            if (key > last) {                               // strictly: an earlier (lower) column keeps a tie
                float cv = key;
                int ci = c;
#pragma unroll
                for (int j = 0; j < BC_MAX_E; ++j) {
                    if (j < E && better(cv, ci, kv[j], ki[j])) {
                        const float tv = kv[j];
                        const int ti = ki[j];
                        kv[j] = cv; ki[j] = ci;
                        cv = tv; ci = ti;
                    }
                }
#pragma unroll
                for (int j = 0; j < BC_MAX_E; ++j) last = j < E ? kv[j] : last;      // kv[E - 1] without a dynamic register index
            }
        }
    }
    const float gm = block_max(m, redf);
    const float zs = block_sum(m == -INFINITY ? 0.f : z * __expf(m - gm), redf);
    const float logz = logf(zs);

    // ---- E rounds of a block arg-max over the lanes' list heads (key descending, column ascending)
    for (int j = 0; j < E; ++j) {
        float bv = kv[0];
        int bi = ki[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sh_v[wave] = bv; sh_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < BC_THREADS / 64; ++w)
                if (better(sh_v[w], sh_i[w], bv, bi)) { bv = sh_v[w]; bi = sh_i[w]; }
            sel[j] = bi;
            redi[0] = bi;
        }
        __syncthreads();
        const int win = redi[0];
        if (win != 0x7fffffff && ki[0] == win) {            // the owner of the winning column pops its head
#pragma unroll
            for (int t = 0; t < BC_MAX_E - 1; ++t) { kv[t] = kv[t + 1]; ki[t] = ki[t + 1]; }
            kv[BC_MAX_E - 1] = -INFINITY;
            ki[BC_MAX_E - 1] = 0x7fffffff;
        }
        __syncthreads();
    }
    if (tid < E) {
        int tok = sel[tid];
        float lp = -INFINITY;                               // fewer than E allowed columns: token 0 at log-probability -inf
        if (tok == 0x7fffffff) tok = 0;
        else lp = (sampled ? src[tok] / temperature : src[tok]) - gm - logz;
        if (raw_tok) raw_tok[(size_t)r * E + tid] = tok;
        if (eos >= 0) {                                     // the EOS rule: an ended beam pads with EOS for free
            const bool ended = row[len - 1] == (int64_t)eos;
            if (ended && lp + log_boost < 0.f) {
                tok = eos;
                lp = 0.f;
            } else {
                lp += log_boost;
            }
        }
        cand_tok[(size_t)r * E + tid] = tok;
        cand_lp[(size_t)r * E + tid] = lp;
    }
}

constexpr int CS_THREADS = 256, CS_MAX_W = 16, CS_MAX_WE = 1024;

// One workgroup per caption: the W survivors of its W x E candidates, then the survivors' id rows and history rows.  Every
// thread owns a set of columns and moves column t of the W parents into column t of the W children through registers, so no
// column is read after it was overwritten.
__global__ __launch_bounds__(CS_THREADS) void beam_consolidate_kernel(const int* __restrict__ cand_tok, const float* __restrict__ cand_lp,
                                                                      float* __restrict__ scores, int64_t* __restrict__ ids, int ids_ld,
                                                                      int* __restrict__ hist, int hist_ld, int* __restrict__ has_eos,
                                                                      int* __restrict__ parent, const int* __restrict__ pos_ptr,
                                                                      const int* __restrict__ len_ptr, int* __restrict__ ctrl, int W, int E,
                                                                      float temperature, int eos, const unsigned* __restrict__ seed,
                                                                      int* __restrict__ raw_pick) {
    __shared__ float tot[CS_MAX_WE], key[CS_MAX_WE];
    __shared__ int taken[CS_MAX_WE];
    __shared__ int pick[CS_MAX_W], par[CS_MAX_W], tok[CS_MAX_W], peos[CS_MAX_W];
    __shared__ float nscore[CS_MAX_W];
    if (ctrl[0]) return;
    const int b = blockIdx.x, tid = threadIdx.x, WE = W * E;
    const int pos = *pos_ptr, len = *len_ptr;
    const int r0 = b * W;
    for (int j = tid; j < WE; j += CS_THREADS) {
        const int w = j / E;
        const float t = scores[r0 + w] + cand_lp[(size_t)(r0 + w) * E + (j - w * E)];
        tot[j] = t;
        key[j] = (temperature > 0.f && t != -INFINITY)
                     ? t / temperature + gumbel(beam_uniform(seed, (unsigned)len, (unsigned)b, (unsigned)j, 1u)) : t;
        taken[j] = 0;
    }
    __syncthreads();
    if (tid < 64) {                                          // W rounds of a wave arg-max (key descending, flat index ascending)
        for (int k = 0; k < W; ++k) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int j = tid; j < WE; j += 64)
                if (!taken[j] && better(key[j], j, bv, bi)) { bv = key[j]; bi = j; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (tid == 0) pick[k] = bi;
            if (bi != 0x7fffffff && (bi & 63) == tid) taken[bi] = 1;    // the lane that scans column bi marks it itself
        }
    }
    __syncthreads();
    if (tid < W) {
        const int j = pick[tid], w = j / E;
        par[tid] = r0 + w;
        tok[tid] = cand_tok[(size_t)(r0 + w) * E + (j - w * E)];
        nscore[tid] = tot[j];
        peos[tid] = has_eos[r0 + w];
        if (raw_pick) raw_pick[r0 + tid] = j;
    }
    __syncthreads();
    int64_t vi[CS_MAX_W];
    for (int t = tid; t < len; t += CS_THREADS) {
#pragma unroll
        for (int w = 0; w < CS_MAX_W; ++w)
            if (w < W) vi[w] = ids[(size_t)par[w] * ids_ld + t];
#pragma unroll
        for (int w = 0; w < CS_MAX_W; ++w)
            if (w < W) ids[(size_t)(r0 + w) * ids_ld + t] = vi[w];
    }
    int vh[CS_MAX_W];
    for (int t = tid; t < pos; t += CS_THREADS) {
#pragma unroll
        for (int w = 0; w < CS_MAX_W; ++w)
            if (w < W) vh[w] = hist[(size_t)par[w] * hist_ld + t];
#pragma unroll
        for (int w = 0; w < CS_MAX_W; ++w)
            if (w < W) hist[(size_t)(r0 + w) * hist_ld + t] = vh[w];
    }
    if (tid < W) {
        const int c = r0 + tid;
        ids[(size_t)c * ids_ld + len] = tok[tid];
        hist[(size_t)c * hist_ld + pos] = par[tid];
        scores[c] = nscore[tid];
        parent[c] = par[tid];
        has_eos[c] = (peos[tid] || (eos >= 0 && tok[tid] == eos)) ? 1 : 0;
    }
    if (tid == 0) {
        bool fin = eos >= 0;
        for (int w = 0; w < W; ++w) fin = fin && (peos[w] || tok[w] == eos);
        if (!fin) atomicAdd(&ctrl[1], 1);
    }
}

// pos / len advance while work remains; the flag is set once no caption is left unfinished, and the counter is cleared for the
// next step
__global__ void beam_advance_kernel(int* counters, int* ctrl) {
    if (threadIdx.x != 0) return;
    if (!ctrl[0]) {
        counters[0] += 1;
        counters[1] += 1;
        if (ctrl[1] == 0) ctrl[0] = 1;
    }
    ctrl[1] = 0;
}

}  // namespace

extern "C" int i2t_beam_candidates(void* stream, const float* logits, int ld, const int64_t* ids, int ids_ld, const int* len_ptr,
                                   const int* ctrl, const int* ngram_sizes, int n_sizes, int R, int V, int E, float temperature, int top_k,
                                   int eos, float log_boost, const unsigned* seed, int* cand_tok, float* cand_lp, int* raw_tok) {
    I2T_REQUIRE(logits && ids && len_ptr && ctrl && seed && cand_tok && cand_lp && R > 0 && V > 0 && (n_sizes == 0 || ngram_sizes),
                "i2t_beam_candidates: bad args");
    I2T_REQUIRE(E >= 1 && E <= BC_MAX_E && E <= V, "i2t_beam_candidates: expansion factor %d (1 .. %d)", E, BC_MAX_E);
    I2T_REQUIRE(ld % 4 == 0 && ld >= ((V + 3) & ~3) && ALIGNED16(logits), "i2t_beam_candidates: logits rows must be 16-byte aligned");
    const size_t lds = (size_t)(V + 31) / 32 * sizeof(unsigned);
    I2T_REQUIRE(lds <= BAN_LDS_MAX, "i2t_beam_candidates: vocabulary %d: the ban bitmap exceeds %d bytes of LDS", V, BAN_LDS_MAX);
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(R), dim3(BC_THREADS), lds, (hipStream_t)stream, logits, ld, ids, ids_ld, len_ptr, ctrl,
                       ngram_sizes, n_sizes, V, E, temperature, top_k, eos, log_boost, seed, cand_tok, cand_lp, raw_tok);
    I2T_CHECK_LAUNCH("i2t_beam_candidates");
    return I2T_OK;
}

extern "C" int i2t_beam_consolidate(void* stream, const int* cand_tok, const float* cand_lp, float* scores, int64_t* ids, int ids_ld,
                                    int* hist, int hist_ld, int* has_eos, int* parent, const int* pos_ptr, const int* len_ptr, int* ctrl,
                                    int B, int W, int E, float temperature, int eos, const unsigned* seed, int* raw_pick) {
    I2T_REQUIRE(cand_tok && cand_lp && scores && ids && hist && has_eos && parent && pos_ptr && len_ptr && ctrl && seed && B > 0,
                "i2t_beam_consolidate: bad args");
    I2T_REQUIRE(W >= 1 && W <= CS_MAX_W && E >= 1 && W * E <= CS_MAX_WE, "i2t_beam_consolidate: beam width %d (1 .. %d), W * E <= %d", W,
                CS_MAX_W, CS_MAX_WE);
    hipLaunchKernelGGL(beam_consolidate_kernel, dim3(B), dim3(CS_THREADS), 0, (hipStream_t)stream, cand_tok, cand_lp, scores, ids, ids_ld,
                       hist, hist_ld, has_eos, parent, pos_ptr, len_ptr, ctrl, W, E, temperature, eos, seed, raw_pick);
    I2T_CHECK_LAUNCH("i2t_beam_consolidate");
    return I2T_OK;
}

extern "C" int i2t_beam_advance(void* stream, int* counters, int* ctrl) {
    I2T_REQUIRE(counters && ctrl, "i2t_beam_advance: bad args");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, ctrl);
    I2T_CHECK_LAUNCH("i2t_beam_advance");
    return I2T_OK;
}
