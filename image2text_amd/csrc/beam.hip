// Beam-search step kernels over the static KV cache (reference models/generation_utils.py:10-148, BeamSearchTokenGenerator).
// R = B * W rows, batch-major (row r = b * W + w).  Every position-dependent input (pos, len, the "all beams ended" flag) lives in
// device memory, so one captured hipGraph replays the whole step once per token with no host round trip:
//   decoder blocks (the HIST attention kernels of decode.hip / family.hip) -> lm_head (fp32 logits) -> i2t_beam_candidates -> i2t_beam_consolidate -> i2t_beam_advance.
// Survivors never copy K/V: a history table hist[R][T] (int32) names the physical cache row that holds key t of beam r.  The step
// writes its new K/V at physical (r, pos); consolidation sets hist[child][t] = hist[parent][t] for t < pos and hist[child][pos] =
// parent.  Each position of each physical row is written once, so no entry a live beam points at is ever overwritten.  A sparse
// layer caches its kept positions only (slot = rank among them): key s of beam r is at (hist[r][slot_pos[s]], s), and a slot
// written again before a kept token lands there is named by no history.
#include "select_common.h"

namespace {

// counter-based uniform in (0, 1) on a grid of 2^-23, a pure function of (seed, step, row, index, salt); image2text_amd/rng.py::beam_uniform
// is the host replica.  salt 0: candidate draws (row = beam row, index = token id); salt 1: consolidation (row = caption, index =
// flat candidate w * E + e).
__device__ __forceinline__ float beam_uniform(const unsigned* seed, unsigned step, unsigned row, unsigned index, unsigned salt) {
    const unsigned h1 = mix32(seed[0] ^ (row * 0x9E3779B9u));
    const unsigned h2 = mix32(h1 + seed[1] + step * 0x85EBCA6Bu + salt * 0x27D4EB2Fu);
    const unsigned h = mix32(h2 + index * 0x165667B1u);
    return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);     // exact in fp32: 23 bits + 1/2
}
// Gumbel noise: key = logit + gumbel; the top-k keys are k draws without replacement, in draw order, from softmax(logits)
__device__ __forceinline__ float gumbel(float u) { return -logf(-logf(u)); }

__device__ __forceinline__ unsigned okey(float f) {            // monotone float -> unsigned (no NaNs on this path)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr int BC_THREADS = 1024, BC_MAX_E = 16;

// One workgroup per beam row.  The row is streamed from the logits (fp32, 16-byte loads, every lane visits its columns in
// ascending order): the top-k threshold by bisection on the order-preserving integer image of the scores (only with a crop, 32
// block-wide counts), then ONE pass that keeps the online max / sum of exp of the scores and a per-lane list of the E best keys
// (raw score or score / T + Gumbel noise; select_common.h's sorted list), merged across the block in E rounds.
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
    const int r = blockIdx.x, tid = threadIdx.x;
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
    topk_clear(kv, ki);
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
                topk_insert(kv, ki, E, key, c);
#pragma unroll
                for (int j = 0; j < BC_MAX_E; ++j) last = j < E ? kv[j] : last;      // kv[E - 1] without a dynamic register index
            }
        }
    }
    const float gm = block_max(m, redf);
    const float zs = block_sum(m == -INFINITY ? 0.f : z * __expf(m - gm), redf);
    const float logz = logf(zs);

    // ---- E rounds of a block arg-max over the lanes' list heads (key descending, column ascending)
    for (int j = 0; j < E; ++j) topk_round<BC_THREADS>(kv, ki, sh_v, sh_i, &redi[0], [&](float, int bi) { sel[j] = bi; });
    if (tid < E) {
        int tok = sel[tid];
        float lp = -INFINITY;                               // fewer than E allowed columns: token 0 at log-probability -inf
        if (tok == TOPK_NONE) tok = 0;
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

// One workgroup per caption: the W survivors of its W x E candidates (wave_rank_rounds), then the survivors' id rows and history
// rows (move_rows: no column is read after it was overwritten).
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
    wave_rank_rounds(key, taken, pick, WE, W);               // (key descending, flat index ascending)
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
    move_rows<CS_MAX_W>(ids, ids_ld, par, r0, W, len, CS_THREADS);
    move_rows<CS_MAX_W>(hist, hist_ld, par, r0, W, pos, CS_THREADS);
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

constexpr int PS_THREADS = 256, PS_MAX_W = 8, PS_MAX_WE = 2 * PS_MAX_W * PS_MAX_W;

// The selection step of generate_captions(num_beams = W) (decoding.beam_pool_select_host is the host replica): one
// workgroup per image, E = 2 W candidates per row.  The top 2 W of the image's W x E totals are ranked (descending, lower flat index
// w * E + e first); a candidate HITS when its token is eos or it is the max_new-th emitted token.  Hits ranked below W are offered to
// the image's pool of finished captions at total / powf(emitted, length_penalty); the pool keeps its W best, sorted, an entry it
// already holds before a new one of the same score.  The first W candidates that do not hit become the running beams.  Pool rows and
// running rows (move_rows) are moved a column at a time through registers -- the pool first, it reads the parents' rows --, so no
// column is read after it was overwritten.  An image closes at the bound, with early_stopping once its pool is full, and without it once the
// best running total / powf(emitted, length_penalty) no longer exceeds the full pool's worst score; a closed image's block returns at
// once, and every open image stores the same 1 into ctrl[1], so the word needs no atomic.
__global__ __launch_bounds__(PS_THREADS) void beam_pool_select_kernel(const int* __restrict__ cand_tok, const float* __restrict__ cand_lp,
                                                                      float* __restrict__ scores, int64_t* __restrict__ ids, int ids_ld,
                                                                      int* __restrict__ hist, int hist_ld, float* __restrict__ tok_lp, int lp_ld,
                                                                      int64_t* __restrict__ pool_ids, float* __restrict__ pool_lp,
                                                                      float* __restrict__ pool_score, float* __restrict__ pool_sum,
                                                                      int* __restrict__ pool_len, int* __restrict__ pool_n, int* __restrict__ closed,
                                                                      const int* __restrict__ pos_ptr, const int* __restrict__ len_ptr,
                                                                      int* __restrict__ ctrl, int W, int P, int max_new, int eos, int pad,
                                                                      float length_penalty, int early_stopping) {
    __shared__ float tot[PS_MAX_WE];
    __shared__ int taken[PS_MAX_WE];
    __shared__ int pick[2 * PS_MAX_W];
    __shared__ int c_par[PS_MAX_W], c_tok[PS_MAX_W];                         // the running children
    __shared__ float c_score[PS_MAX_W], c_lp[PS_MAX_W];
    __shared__ int e_src[PS_MAX_W + 1], e_par[PS_MAX_W + 1], e_tok[PS_MAX_W + 1], e_len[PS_MAX_W + 1];      // the pool after the merge; src >= 0:
    __shared__ float e_score[PS_MAX_W + 1], e_sum[PS_MAX_W + 1], e_lp[PS_MAX_W + 1];                         // the row it held, -1: a new one
    __shared__ int flags[2];                                                  // [the pool changed, the image closes]
    if (ctrl[0]) return;
    const int b = blockIdx.x, tid = threadIdx.x, E = 2 * W, WE = W * E;
    if (closed[b]) return;
    const int pos = *pos_ptr, len = *len_ptr;
    if (len < P || len >= P + max_new || pos < 0 || pos >= hist_ld) return;   // counters outside the call's columns: nothing is written
    const int r0 = b * W, total_cols = P + max_new;
    for (int j = tid; j < WE; j += PS_THREADS) {
        const int w = j / E;
        tot[j] = scores[r0 + w] + cand_lp[(size_t)(r0 + w) * E + (j - w * E)];
        taken[j] = 0;
    }
    __syncthreads();
    wave_rank_rounds(tot, taken, pick, WE, E);               // (total descending, flat index ascending)
    __syncthreads();
    if (tid == 0) {
        const int emitted = len + 1 - P;
        const bool bound = emitted >= max_new;
        const float denom = powf((float)emitted, length_penalty);
        int m = pool_n[b], nchild = 0, changed = 0;
        for (int i = 0; i < W; ++i) {
            e_src[i] = i;
            e_score[i] = pool_score[r0 + i];
            e_sum[i] = pool_sum[r0 + i];
            e_len[i] = pool_len[r0 + i];
        }
        for (int k = 0; k < E; ++k) {
            const int j = pick[k];
            if (j == TOPK_NONE) continue;                   // NaN totals only: nothing ranks
            const int w = j / E;
            const int tk = cand_tok[(size_t)(r0 + w) * E + (j - w * E)];
            const float lpv = cand_lp[(size_t)(r0 + w) * E + (j - w * E)];
            if (bound || (eos >= 0 && tk == eos)) {
                if (k >= W) continue;
                const float s = tot[j] / denom;
                int at = 0;
                while (at < m && e_score[at] >= s) ++at;     // behind everything at least as good
                if (at >= W) continue;
                for (int i = (m < W ? m : W - 1); i > at; --i) {
                    e_src[i] = e_src[i - 1]; e_par[i] = e_par[i - 1]; e_tok[i] = e_tok[i - 1]; e_len[i] = e_len[i - 1];
                    e_score[i] = e_score[i - 1]; e_sum[i] = e_sum[i - 1]; e_lp[i] = e_lp[i - 1];
                }
                e_src[at] = -1; e_par[at] = r0 + w; e_tok[at] = tk; e_len[at] = len + 1;
                e_score[at] = s; e_sum[at] = tot[j]; e_lp[at] = lpv;
                if (m < W) ++m;
                changed = 1;
            } else if (nchild < W) {
                c_par[nchild] = r0 + w; c_tok[nchild] = tk; c_score[nchild] = tot[j]; c_lp[nchild] = lpv;
                ++nchild;
            }
        }
        for (int w = nchild; w < W; ++w) {                   // fewer than W live candidates (NaN or repeated-EOS inputs only): the row stays, dead
            c_par[w] = r0 + w; c_tok[w] = pad; c_score[w] = -INFINITY; c_lp[w] = 0.f;
        }
        for (int i = m; i < W; ++i) e_src[i] = i;            // slots past the pool's count keep what they hold
        int cl = bound ? 1 : 0;
        if (!cl && m == W) cl = early_stopping ? 1 : (c_score[0] / denom > e_score[W - 1] ? 0 : 1);
        for (int i = 0; i < m; ++i) {
            pool_score[r0 + i] = e_score[i];
            pool_sum[r0 + i] = e_sum[i];
            pool_len[r0 + i] = e_len[i];
        }
        pool_n[b] = m;
        closed[b] = cl;
        if (!cl) ctrl[1] = 1;
        flags[0] = changed;
        flags[1] = cl;
    }
    __syncthreads();
    if (flags[0]) {                                          // the pool's rows: a kept row from the slot it held, a new one from its parent
        int64_t vi[PS_MAX_W];
        float vf[PS_MAX_W];
        for (int t = tid; t < total_cols; t += PS_THREADS) {
#pragma unroll
            for (int w = 0; w < PS_MAX_W; ++w)
                if (w < W) {
                    const int s = e_src[w];
                    if (s >= 0) {
                        vi[w] = pool_ids[(size_t)(r0 + s) * ids_ld + t];
                        vf[w] = pool_lp[(size_t)(r0 + s) * lp_ld + t];
                    } else if (t < len) {
                        vi[w] = ids[(size_t)e_par[w] * ids_ld + t];
                        vf[w] = tok_lp[(size_t)e_par[w] * lp_ld + t];
                    } else {
                        vi[w] = t == len ? (int64_t)e_tok[w] : (int64_t)pad;
                        vf[w] = t == len ? e_lp[w] : 0.f;
                    }
                }
#pragma unroll
            for (int w = 0; w < PS_MAX_W; ++w)
                if (w < W) {
                    pool_ids[(size_t)(r0 + w) * ids_ld + t] = vi[w];
                    pool_lp[(size_t)(r0 + w) * lp_ld + t] = vf[w];
                }
        }
    }
    __syncthreads();
    if (flags[1] && len + 1 >= total_cols) return;           // at the bound nothing runs on: the rows stay
    move_rows<PS_MAX_W>(ids, ids_ld, c_par, r0, W, len, PS_THREADS);
    move_rows<PS_MAX_W>(tok_lp, lp_ld, c_par, r0, W, len, PS_THREADS);
    move_rows<PS_MAX_W>(hist, hist_ld, c_par, r0, W, pos, PS_THREADS);
    if (tid < W) {
        const int c = r0 + tid;
        ids[(size_t)c * ids_ld + len] = c_tok[tid];
        tok_lp[(size_t)c * lp_ld + len] = c_lp[tid];
        hist[(size_t)c * hist_ld + pos] = c_par[tid];
        scores[c] = c_score[tid];
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

extern "C" int i2t_beam_pool_select(void* stream, const int* cand_tok, const float* cand_lp, float* scores, int64_t* ids, int ids_ld, int* hist,
                                    int hist_ld, float* tok_lp, int lp_ld, int64_t* pool_ids, float* pool_lp, float* pool_score,
                                    float* pool_sum, int* pool_len, int* pool_n, int* closed, const int* pos_ptr, const int* len_ptr,
                                    int* ctrl, int B, int W, int P, int max_new, int eos, int pad, float length_penalty,
                                    int early_stopping) {
    I2T_REQUIRE(cand_tok && cand_lp && scores && ids && hist && tok_lp && pool_ids && pool_lp && pool_score && pool_sum && pool_len &&
                    pool_n && closed && pos_ptr && len_ptr && ctrl && B > 0,
                "i2t_beam_pool_select: bad args");
    I2T_REQUIRE(W >= 1 && W <= PS_MAX_W, "i2t_beam_pool_select: beam width %d (1 .. %d)", W, PS_MAX_W);
    I2T_REQUIRE(P >= 1 && max_new >= 1 && pad >= 0, "i2t_beam_pool_select: P = %d, max_new = %d (each at least 1), pad = %d (at least 0)", P,
                max_new, pad);
    I2T_REQUIRE((long)P + max_new <= ids_ld && (long)P + max_new <= lp_ld && hist_ld >= 1,
                "i2t_beam_pool_select: P + max_new = %ld columns exceed ids_ld = %d or lp_ld = %d (hist_ld = %d)", (long)P + max_new, ids_ld,
                lp_ld, hist_ld);
    // the exponent bits, not a comparison: no fast-math folding of a NaN test
    I2T_REQUIRE((__builtin_bit_cast(unsigned, length_penalty) & 0x7f800000u) != 0x7f800000u && (early_stopping == 0 || early_stopping == 1),
                "i2t_beam_pool_select: length_penalty must be finite and early_stopping 0 or 1 (%d)", early_stopping);
    hipLaunchKernelGGL(beam_pool_select_kernel, dim3(B), dim3(PS_THREADS), 0, (hipStream_t)stream, cand_tok, cand_lp, scores, ids, ids_ld, hist,
                       hist_ld, tok_lp, lp_ld, pool_ids, pool_lp, pool_score, pool_sum, pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, W, P,
                       max_new, eos, pad, length_penalty, early_stopping);
    I2T_CHECK_LAUNCH("i2t_beam_pool_select");
    return I2T_OK;
}

extern "C" int i2t_beam_advance(void* stream, int* counters, int* ctrl) {
    I2T_REQUIRE(counters && ctrl, "i2t_beam_advance: bad args");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, ctrl);
    I2T_CHECK_LAUNCH("i2t_beam_advance");
    return I2T_OK;
}
