// Closed-set decoding of generate_captions(phrases=...): a pre-pass and a post-pass around the fp32-logits choosers of a
// caption step, which run between them as they are.  The phrase set is a flat CSR trie in device memory (decoding.phrase_trie): the
// children of node n are edges child_off[n] .. child_off[n + 1), child_tok ascending, child_next the node an edge leads to, term[n] the
// index of the phrase that ends at n or -1; node 0 is the root.  Every row keeps its node in node[r].  Plain loads and vector stores,
// no atomics; nothing is read or written once *done is set.
#include "select_common.h"

namespace {

// The edges of node nd, clipped to what the buffers hold: `edges` entries of child_tok / child_next and kept_ld - 1 gathers per row (the
// host sizes both from the trie, so nothing is clipped on a trie that phrase_trie built).
__device__ __forceinline__ void node_edges(const int* __restrict__ child_off, int nd, int edges, int cap, int& off, int& fan) {
    off = child_off[nd];
    fan = child_off[nd + 1] - off;
    if (off < 0 || off > edges) {
        off = 0;
        fan = 0;
    }
    fan = min(fan, min(edges - off, cap));
    fan = fan < 0 ? 0 : fan;
}

// The pre-pass, between the lm_head GEMM and the chooser: one workgroup per row.  Pass A: the RAW row's log-sum-exp
// (select_common.h's row_lse_partials / lse_waves_merge: bit-reproducible) -> raw_lse[r]; in the same pass
// kept[r][i] = z[child_tok[off + i]] for the node's children and kept[r][fan] = z[eos] at a terminal node, all raw since nothing has
// been written.  Barrier.  Pass B: -inf over columns [0, V), 16-byte stores; columns V .. ld are not touched.  Barrier.  Pass C: the
// kept values back into their columns (thread i of pass A wrote kept[r][i] and reads it here itself).  Any fan-out works: no LDS bitmap,
// no limit on V.  decoding.trie_mask_host is the host's statement of what the row holds afterwards.
// RAGGED (i2t_caption_trie_mask_ragged): row r belongs to image r / N, and while *len_ptr < plen[r / N] the row sits in
// a forced prompt column: its workgroup returns before it reads or writes anything of the row -- the logits stay raw, raw_lse[r] and
// kept[r] keep what they held.  Every other row runs the body below unchanged.
constexpr int TRIE_THREADS = 256;
template <bool RAGGED>
__global__ __launch_bounds__(TRIE_THREADS) void caption_trie_mask_kernel(float* logits, int ld, const int* __restrict__ node,
                                                                         const int* __restrict__ child_off, const int* __restrict__ child_tok,
                                                                         const int* __restrict__ term, int nodes, int edges, int eos,
                                                                         const int* __restrict__ done, float* __restrict__ raw_lse, float* kept,
                                                                         int kept_ld, int V, const int* __restrict__ len_ptr,
                                                                         const int* __restrict__ plen, int N) {
    __shared__ float rmx[TRIE_THREADS / 64], rse[TRIE_THREADS / 64];
    if (*done) return;                                  // block-uniform, before any barrier
    const int r = blockIdx.x, tid = threadIdx.x;
    if (RAGGED && *len_ptr < plen[r / N]) return;       // block-uniform: a forced column
    const int nd = node[r];
    if (nd < 0 || nd >= nodes) return;                  // block-uniform (never from the advance kernel)
    int off, fan;
    node_edges(child_off, nd, edges, kept_ld - 1, off, fan);
    const bool terminal = term[nd] >= 0;
    float* z = logits + (size_t)r * ld;
    float* kp = kept + (size_t)r * kept_ld;
    float mx, se;
    row_lse_partials<TRIE_THREADS>(z, V, mx, se, rmx, rse);
    for (int i = tid; i < fan; i += TRIE_THREADS) {
        const int t = child_tok[off + i];
        kp[i] = (t >= 0 && t < V) ? z[t] : -INFINITY;
    }
    if (tid == 0 && terminal) kp[fan] = z[eos];
    __syncthreads();                                    // every read of the raw row is done
    if (tid == 0) raw_lse[r] = lse_waves_merge<TRIE_THREADS>(mx, se, rmx, rse);
    const int vend = V & ~3;                            // (ld % 4 == 0 and a 16-byte base: the entry point's checks)
    const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int c4 = tid * 4; c4 < vend; c4 += TRIE_THREADS * 4) *reinterpret_cast<f32x4*>(z + c4) = ninf;
    for (int c = vend + tid; c < V; c += TRIE_THREADS) z[c] = -INFINITY;
    __syncthreads();                                    // the row is -inf before an allowed column gets its value back
    for (int i = tid; i < fan; i += TRIE_THREADS) {
        const int t = child_tok[off + i];
        if (t >= 0 && t < V) z[t] = kp[i];              // this thread's own store of pass A
    }
    if (tid == 0 && terminal) z[eos] = kp[fan];
}

// The post-pass, between the chooser and i2t_caption_finish: one wave per row.  A finished row is skipped.  With c = ids[r][len] the
// chosen token: EOS at a terminal node names the row's phrase, phrase_index[r] = term[node]; a child moves the row, node[r] =
// child_next (the lanes stride over the node's sorted children; at most one matches); either way tok_lp[r][len] = logits[r][c] -
// raw_lse[r] over what the chooser wrote there -- the allowed columns hold their raw values after the pre-pass, so this is the raw
// row's log_softmax at c.  Any other token (never from a chooser) leaves node and log-prob as they were.
// RAGGED (i2t_caption_trie_advance_ragged): a row in a forced column (len < plen[r / N]) is skipped like a finished one -- node,
// phrase_index and tok_lp[r][len] stay; i2t_caption_finish_ragged replaces the chooser's token and log-prob after this kernel.
constexpr int TRIE_ADV_WAVES = 4;
template <bool RAGGED>
__global__ __launch_bounds__(64 * TRIE_ADV_WAVES) void caption_trie_advance_kernel(const int64_t* __restrict__ ids, int ids_ld,
                                                                                   const int* __restrict__ len_ptr, const int* __restrict__ finished,
                                                                                   const float* __restrict__ logits, int ld,
                                                                                   const float* __restrict__ raw_lse, const int* __restrict__ child_off,
                                                                                   const int* __restrict__ child_tok, const int* __restrict__ child_next,
                                                                                   const int* __restrict__ term, int nodes, int edges, int eos,
                                                                                   const int* __restrict__ done, int* __restrict__ node,
                                                                                   int* __restrict__ phrase_index, float* __restrict__ tok_lp, int lp_ld,
                                                                                   int R, int V, const int* __restrict__ plen, int N) {
    if (*done) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * TRIE_ADV_WAVES + (threadIdx.x >> 6);
    const int len = *len_ptr;
    if (r >= R || len < 0 || len >= ids_ld || len >= lp_ld) return;      // wave-uniform, as every return below
    if (finished[r]) return;
    if (RAGGED && len < plen[r / N]) return;                             // a forced column
    const int64_t c = ids[(size_t)r * ids_ld + len];
    const int nd = node[r];
    if (c < 0 || c >= V || nd < 0 || nd >= nodes) return;
    float* lp = tok_lp + (size_t)r * lp_ld + len;
    if (c == (int64_t)eos) {
        const int p = term[nd];
        if (p >= 0 && lane == 0) {
            phrase_index[r] = p;
            *lp = logits[(size_t)r * ld + c] - raw_lse[r];
        }
        return;
    }
    int off, fan;
    node_edges(child_off, nd, edges, edges, off, fan);
    int nxt = -1;
    for (int i = lane; i < fan; i += 64)
        if (child_tok[off + i] == (int)c) nxt = child_next[off + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nxt = max(nxt, __shfl_xor(nxt, o, 64));
    if (nxt < 0 || nxt >= nodes) return;
    if (lane == 0) {
        node[r] = nxt;
        *lp = logits[(size_t)r * ld + c] - raw_lse[r];
    }
}

// ---- Exact closed-set scoring (score_phrases): the trie is walked level by level, every node of a level a row, nothing
// pruned.  The level tables are host-built (decoding.trie_levels) and static.

// The RAW row's log-sum-exp alone, for the fp32-logits head: select_common.h's row_lse_partials / lse_waves_merge, as
// caption_trie_mask_kernel's pass A, and nothing else: one workgroup per row, bit-reproducible, the row is only read.
__global__ __launch_bounds__(TRIE_THREADS) void rows_lse_kernel(const float* __restrict__ logits, int ld, float* __restrict__ lse, int V) {
    __shared__ float rmx[TRIE_THREADS / 64], rse[TRIE_THREADS / 64];
    const int r = blockIdx.x;
    float mx, se;
    row_lse_partials<TRIE_THREADS>(logits + (size_t)r * ld, V, mx, se, rmx, rse);
    __syncthreads();
    if (threadIdx.x == 0) lse[r] = lse_waves_merge<TRIE_THREADS>(mx, se, rmx, rse);
}

// One level of the walk, after the level's step and its rows' LSE: one wave per (image b, entry j).  The first B * n_child waves are
// the CHILD part: row b * W + j of the next level takes the node whose parent sits in row p = child_parent[j] and whose token is
// k = child_tok[j]: path_out[b W + j] = path_in[b W + p] + (z - lse[b W + p]) in exactly this order, ids[b W + j][len] = k.  The other
// B * n_term waves are the TERMINAL part: row p = term_row[j] of THIS level holds a node that ends a phrase, and every phrase index i
// of term_phrase[term_off[j] .. term_off[j + 1]) (the node's duplicates) gets logprob[b][i] = path_in[b W + p] + (z_eos - lse[b W + p]).
// z is logits[row][k] when a logits pointer is given, else scale . hidden[row] . w_head[k] re-evaluated in fp32 from the bf16 operands
// as lse_token_logprob_kernel does (lane l the 8-element groups l, l + 64, ..., a fixed xor tree; the scale one rounded multiply, kept
// out of the subtraction).  path_in and path_out are two buffers: no cell is read and written in one launch.  An entry whose parent row
// or token lies outside its range (never from decoding.trie_levels) writes nothing, and so does a column outside the id rows.
constexpr int EXPAND_WAVES = 4;

// What one wave of a level-expand kernel computes for the token `tok` behind the node in row `pr`: path_in[pr] + (z - lse[pr]), z as
// above.  Every lane returns the value.  trie_level_expand_kernel and trie_level_expand_sets_kernel both call it: one statement of the
// arithmetic.
__device__ __forceinline__ float expand_value(const bf16_t* __restrict__ hid, int ld_h, const bf16_t* __restrict__ Wh, int ldw, int d, float scale,
                                              const float* __restrict__ logits, int ld, const float* __restrict__ lse,
                                              const float* __restrict__ path_in, size_t pr, int tok, int lane) {
    float z;
    if (logits != nullptr) {
        z = logits[pr * ld + tok];
    } else {
        const bf16_t* wr = Wh + (size_t)tok * ldw;
        const bf16_t* hr = hid + pr * ld_h;
        float acc = 0.f;
        for (int k = 8 * lane; k < d; k += 8 * 64) {
            const u32x4 wq = *reinterpret_cast<const u32x4*>(wr + k), hq = *reinterpret_cast<const u32x4*>(hr + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += bf16lo(wq[e]) * bf16lo(hq[e]) + bf16hi(wq[e]) * bf16hi(hq[e]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        z = __fmul_rn(scale, acc);                           // its own rounding: never fused into the subtraction below
    }
    return path_in[pr] + (z - lse[pr]);
}

// The terminal part's stores: v into lp[i] for every phrase index i of term_phrase[term_off[j] .. term_off[j + 1]), the range clipped to
// the n_term_phrases entries the table holds and an index outside [0, kmax) skipped.
__device__ __forceinline__ void expand_terminal_store(const int* __restrict__ term_off, const int* __restrict__ term_phrase, int j,
                                                      int n_term_phrases, float* __restrict__ lp, int kmax, float v, int lane) {
    int lo = term_off[j], hi = term_off[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_term_phrases ? n_term_phrases : hi;
    for (int i = lo + lane; i < hi; i += 64) {
        const int ph = term_phrase[i];
        if (ph >= 0 && ph < kmax) lp[ph] = v;
    }
}

__global__ __launch_bounds__(64 * EXPAND_WAVES) void trie_level_expand_kernel(
    const bf16_t* __restrict__ hid, int ld_h, const bf16_t* __restrict__ Wh, int ldw, int d, float scale, const float* __restrict__ logits, int ld,
    const float* __restrict__ lse, const float* __restrict__ path_in, float* __restrict__ path_out, const int* __restrict__ child_parent,
    const int* __restrict__ child_tok, int n_child, const int* __restrict__ term_row, const int* __restrict__ term_off,
    const int* __restrict__ term_phrase, int n_term, int n_term_phrases, int64_t* __restrict__ ids, int ids_ld, const int* __restrict__ len_ptr,
    float* __restrict__ logprob, int lp_ld, int eos, int B, int W, int V) {
    const int lane = threadIdx.x & 63;
    const long wv = (long)blockIdx.x * EXPAND_WAVES + (threadIdx.x >> 6);
    const long n_exp = (long)B * n_child, total = n_exp + (long)B * n_term;
    if (wv >= total) return;                                 // wave-uniform, as every return below
    const bool child = wv < n_exp;
    int b, j, p, tok;
    if (child) {
        b = (int)(wv / n_child);
        j = (int)(wv % n_child);
        p = child_parent[j];
        tok = child_tok[j];
    } else {
        b = (int)((wv - n_exp) / n_term);
        j = (int)((wv - n_exp) % n_term);
        p = term_row[j];
        tok = eos;
    }
    if (p < 0 || p >= W || tok < 0 || tok >= V) return;
    const size_t pr = (size_t)b * W + p;
    const float v = expand_value(hid, ld_h, Wh, ldw, d, scale, logits, ld, lse, path_in, pr, tok, lane);
    if (child) {
        const int len = *len_ptr;
        if (len < 0 || len >= ids_ld) return;
        if (lane == 0) {
            const size_t c = (size_t)b * W + j;
            path_out[c] = v;
            ids[c * ids_ld + len] = tok;
        }
        return;
    }
    expand_terminal_store(term_off, term_phrase, j, n_term_phrases, logprob + (size_t)b * lp_ld, lp_ld, v, lane);
}

// i2t_trie_level_expand_sets: one launch in which the images stand at different levels of different tries, or in a
// forced prompt column, or behind their last level.  The level tables of every (set, level) lie end to end in child_parent / child_tok
// [n_child_all], term_row [n_term_all], term_off [n_off_all] (a level's n_term + 1 offsets, which index term_phrase [n_term_phrases]
// absolutely).  Image b's state is the 8 int32 of img + 8 b (IMG_* below), host-built per step.  One wave per (image, entry): the first
// B * e_child waves are the child part, entry j of image b; the other B * e_term the terminal part.
//   level < 0, forced token k >= 0 (child part, j < W): ids[b W + j][col] = k and path_out[b W + j] = path_in[b W + j] -- the swap stays
//     valid; nothing is scored.  level < 0 and k < 0: the image is finished, nothing of it is read or written.
//   level >= 0: entry j < n of the image's own table range does exactly what trie_level_expand_kernel does with it (expand_value, then
//     the same stores), the terminal part into the image's own logprob row of kmax columns.
// An entry outside its image's range, a range outside the tables, a column outside the id rows: nothing is written.
constexpr int IMG_LEVEL = 0, IMG_FORCED = 1, IMG_CHILD_AT = 2, IMG_N_CHILD = 3, IMG_TERM_AT = 4, IMG_N_TERM = 5, IMG_OFF_AT = 6, IMG_COL = 7,
              IMG_INTS = 8;
__global__ __launch_bounds__(64 * EXPAND_WAVES) void trie_level_expand_sets_kernel(
    const bf16_t* __restrict__ hid, int ld_h, const bf16_t* __restrict__ Wh, int ldw, int d, float scale, const float* __restrict__ logits, int ld,
    const float* __restrict__ lse, const float* __restrict__ path_in, float* __restrict__ path_out, const int* __restrict__ child_parent,
    const int* __restrict__ child_tok, int n_child_all, const int* __restrict__ term_row, int n_term_all, const int* __restrict__ term_off,
    int n_off_all, const int* __restrict__ term_phrase, int n_term_phrases, const int* __restrict__ img, int e_child, int e_term,
    int64_t* __restrict__ ids, int ids_ld, float* __restrict__ logprob, int lp_ld, int kmax, int eos, int B, int W, int V) {
    const int lane = threadIdx.x & 63;
    const long wv = (long)blockIdx.x * EXPAND_WAVES + (threadIdx.x >> 6);
    const long n_exp = (long)B * e_child, total = n_exp + (long)B * e_term;
    if (wv >= total) return;                                 // wave-uniform, as every return below
    const bool child = wv < n_exp;
    const int b = child ? (int)(wv / e_child) : (int)((wv - n_exp) / e_term);
    const int j = child ? (int)(wv % e_child) : (int)((wv - n_exp) % e_term);
    const int* st = img + (size_t)b * IMG_INTS;
    const int col = st[IMG_COL];
    if (st[IMG_LEVEL] < 0) {                                 // a forced column, or a finished image
        const int k = st[IMG_FORCED];
        if (!child || k < 0 || k >= V || j >= W || col < 0 || col >= ids_ld) return;
        if (lane == 0) {
            const size_t r = (size_t)b * W + j;
            path_out[r] = path_in[r];
            ids[r * ids_ld + col] = k;
        }
        return;
    }
    int p, tok, at;
    if (child) {
        const int n = st[IMG_N_CHILD];
        at = st[IMG_CHILD_AT];
        if (j >= n || at < 0 || at > n_child_all - n) return;
        p = child_parent[at + j];
        tok = child_tok[at + j];
    } else {
        const int n = st[IMG_N_TERM], off = st[IMG_OFF_AT];
        at = st[IMG_TERM_AT];
        if (j >= n || at < 0 || at > n_term_all - n || off < 0 || off > n_off_all - n - 1) return;
        p = term_row[at + j];
        tok = eos;
        at = off;
    }
    if (p < 0 || p >= W || tok < 0 || tok >= V) return;
    const size_t pr = (size_t)b * W + p;
    const float v = expand_value(hid, ld_h, Wh, ldw, d, scale, logits, ld, lse, path_in, pr, tok, lane);
    if (child) {
        if (col < 0 || col >= ids_ld) return;
        if (lane == 0) {
            const size_t c = (size_t)b * W + j;
            path_out[c] = v;
            ids[c * ids_ld + col] = tok;
        }
        return;
    }
    expand_terminal_store(term_off + at, term_phrase, j, n_term_phrases, logprob + (size_t)b * lp_ld, kmax, v, lane);
}

}  // namespace

namespace {

// Three checks every entry point of this file that takes the operand makes; `fn` names the caller in the message.
int check_trie_tables(const char* fn, int nodes, int edges) {
    I2T_REQUIRE(nodes >= 1 && edges >= 0, "%s: nodes = %d, edges = %d: a trie has a root", fn, nodes, edges);
    return I2T_OK;
}
int check_eos_in_vocab(const char* fn, int eos, int V) {
    I2T_REQUIRE(eos >= 0 && eos < V, "%s: eos = %d outside the vocabulary of %d", fn, eos, V);
    return I2T_OK;
}
int check_logits_rows(const char* fn, int ld, int V) {                  // fp32 rows the kernels read in 16-byte groups
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "%s: ld = %d: logits rows hold V = %d columns and start on 16 bytes", fn, ld, V);
    return I2T_OK;
}
#define TRIE_TRY(call)                    \
    do {                                  \
        if (int rc_ = (call)) return rc_; \
    } while (0)

// The checks and the launch the plain and the ragged entry point share; `fn` names the caller in every message.  plen null: the plain
// kernel, which reads neither len_ptr nor N.
int trie_mask_launch(const char* fn, void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                     const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept, int kept_ld, int R, int V,
                     const int* len_ptr, const int* plen, int N) {
    I2T_REQUIRE(logits && node && child_off && child_tok && term && done && raw_lse && kept, "%s: null pointer", fn);
    I2T_REQUIRE(R > 0 && V > 0, "%s: R = %d rows, V = %d", fn, R, V);
    TRIE_TRY(check_logits_rows(fn, ld, V));
    TRIE_TRY(check_eos_in_vocab(fn, eos, V));
    TRIE_TRY(check_trie_tables(fn, nodes, edges));
    I2T_REQUIRE(kept_ld >= 1, "%s: kept_ld = %d: a row keeps at least the EOS logit", fn, kept_ld);
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(kept) && ALIGNED16(raw_lse) && ALIGNED16(node) && ALIGNED16(child_off) && ALIGNED16(child_tok) &&
                    ALIGNED16(term),
                "%s: misaligned base pointer (16 bytes)", fn);
    if (plen)
        hipLaunchKernelGGL(caption_trie_mask_kernel<true>, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, node, child_off,
                           child_tok, term, nodes, edges, eos, done, raw_lse, kept, kept_ld, V, len_ptr, plen, N);
    else
        hipLaunchKernelGGL(caption_trie_mask_kernel<false>, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, node, child_off,
                           child_tok, term, nodes, edges, eos, done, raw_lse, kept, kept_ld, V, nullptr, nullptr, 1);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

int trie_advance_launch(const char* fn, void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                        const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok, const int* child_next,
                        const int* term, int nodes, int edges, int eos, const int* done, int* node, int* phrase_index, float* tok_lp, int lp_ld,
                        int R, int V, const int* plen, int N) {
    I2T_REQUIRE(ids && len_ptr && finished && logits && raw_lse && child_off && child_tok && child_next && term && done && node && phrase_index &&
                    tok_lp,
                "%s: null pointer", fn);
    I2T_REQUIRE(R > 0 && V > 0 && ids_ld > 0 && lp_ld > 0, "%s: R = %d rows, V = %d, ids_ld = %d, lp_ld = %d", fn, R, V, ids_ld, lp_ld);
    TRIE_TRY(check_logits_rows(fn, ld, V));
    TRIE_TRY(check_eos_in_vocab(fn, eos, V));
    TRIE_TRY(check_trie_tables(fn, nodes, edges));
    I2T_REQUIRE(ALIGNED16(ids) && ALIGNED16(logits) && ALIGNED16(raw_lse) && ALIGNED16(node) && ALIGNED16(phrase_index) && ALIGNED16(child_off) &&
                    ALIGNED16(child_tok) && ALIGNED16(child_next) && ALIGNED16(term),
                "%s: misaligned base pointer (16 bytes)", fn);
    const dim3 grid((R + TRIE_ADV_WAVES - 1) / TRIE_ADV_WAVES), block(64 * TRIE_ADV_WAVES);
    if (plen)
        hipLaunchKernelGGL(caption_trie_advance_kernel<true>, grid, block, 0, (hipStream_t)stream, ids, ids_ld, len_ptr, finished, logits, ld,
                           raw_lse, child_off, child_tok, child_next, term, nodes, edges, eos, done, node, phrase_index, tok_lp, lp_ld, R, V, plen,
                           N);
    else
        hipLaunchKernelGGL(caption_trie_advance_kernel<false>, grid, block, 0, (hipStream_t)stream, ids, ids_ld, len_ptr, finished, logits, ld,
                           raw_lse, child_off, child_tok, child_next, term, nodes, edges, eos, done, node, phrase_index, tok_lp, lp_ld, R, V,
                           nullptr, 1);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

}  // namespace

extern "C" int i2t_caption_trie_mask(void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                                     const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept, int kept_ld,
                                     int R, int V) {
    return trie_mask_launch("i2t_caption_trie_mask", stream, logits, ld, node, child_off, child_tok, term, nodes, edges, eos, done, raw_lse, kept,
                            kept_ld, R, V, nullptr, nullptr, 1);
}

extern "C" int i2t_caption_trie_mask_ragged(void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                                            const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept,
                                            int kept_ld, const int* len_ptr, const int* plen, int N, int R, int V) {
    I2T_REQUIRE(N >= 1, "i2t_caption_trie_mask_ragged: N = %d rows per image (at least 1)", N);
    I2T_REQUIRE(R % N == 0, "i2t_caption_trie_mask_ragged: R = %d rows are not whole groups of N = %d", R, N);
    I2T_REQUIRE(plen && len_ptr, "i2t_caption_trie_mask_ragged: null plen or len_ptr: the prompt lengths are device memory");
    I2T_REQUIRE(ALIGNED16(plen), "i2t_caption_trie_mask_ragged: misaligned plen (16 bytes)");
    return trie_mask_launch("i2t_caption_trie_mask_ragged", stream, logits, ld, node, child_off, child_tok, term, nodes, edges, eos, done, raw_lse,
                            kept, kept_ld, R, V, len_ptr, plen, N);
}

extern "C" int i2t_caption_trie_advance(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                                        const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok,
                                        const int* child_next, const int* term, int nodes, int edges, int eos, const int* done, int* node,
                                        int* phrase_index, float* tok_lp, int lp_ld, int R, int V) {
    return trie_advance_launch("i2t_caption_trie_advance", stream, ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok,
                               child_next, term, nodes, edges, eos, done, node, phrase_index, tok_lp, lp_ld, R, V, nullptr, 1);
}

extern "C" int i2t_caption_trie_advance_ragged(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                                               const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok,
                                               const int* child_next, const int* term, int nodes, int edges, int eos, const int* done,
                                               int* node, int* phrase_index, float* tok_lp, int lp_ld, const int* plen, int N, int R, int V) {
    I2T_REQUIRE(N >= 1, "i2t_caption_trie_advance_ragged: N = %d rows per image (at least 1)", N);
    I2T_REQUIRE(R % N == 0, "i2t_caption_trie_advance_ragged: R = %d rows are not whole groups of N = %d", R, N);
    I2T_REQUIRE(plen, "i2t_caption_trie_advance_ragged: null plen: the prompt lengths are device memory");
    I2T_REQUIRE(ALIGNED16(plen), "i2t_caption_trie_advance_ragged: misaligned plen (16 bytes)");
    return trie_advance_launch("i2t_caption_trie_advance_ragged", stream, ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off,
                               child_tok, child_next, term, nodes, edges, eos, done, node, phrase_index, tok_lp, lp_ld, R, V, plen, N);
}

extern "C" int i2t_rows_lse(void* stream, const float* logits, int ld, float* lse, int R, int V) {
    I2T_REQUIRE(logits && lse, "i2t_rows_lse: null pointer");
    I2T_REQUIRE(R > 0 && V > 0, "i2t_rows_lse: R = %d rows, V = %d", R, V);
    TRIE_TRY(check_logits_rows("i2t_rows_lse", ld, V));
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(lse), "i2t_rows_lse: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(rows_lse_kernel, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, lse, V);
    I2T_CHECK_LAUNCH("i2t_rows_lse");
    return I2T_OK;
}

namespace {

// What i2t_trie_level_expand and i2t_trie_level_expand_sets both hold their EOS, their two path buffers and their z operands to, in
// this order; `fn` names the caller in every message.
int check_expand_operands(const char* fn, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d, float scale,
                          const float* logits, int ld, const float* path_in, const float* path_out, int eos, int V) {
    (void)hidden, (void)w_head;
    TRIE_TRY(check_eos_in_vocab(fn, eos, V));
    I2T_REQUIRE(path_in != path_out, "%s: path_in and path_out are one buffer: they swap each level", fn);
    if (logits) {
        TRIE_TRY(check_logits_rows(fn, ld, V));
    } else {
        I2T_REQUIRE(d > 0 && d % 8 == 0 && ld_hidden >= d && ld_w >= d && ld_hidden % 8 == 0 && ld_w % 8 == 0,
                    "%s: d = %d must be a multiple of 8, hidden / head rows (ld %d / %d) 16-byte aligned", fn, d, ld_hidden, ld_w);
        I2T_REQUIRE(scale == scale && scale - scale == 0.f, "%s: scale must be finite", fn);
    }
    return I2T_OK;
}

}  // namespace

extern "C" int i2t_trie_level_expand(void* stream, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d, float scale,
                                     const float* logits, int ld, const float* lse, const float* path_in, float* path_out,
                                     const int* child_parent, const int* child_tok, int n_child, const int* term_row, const int* term_off,
                                     const int* term_phrase, int n_term, int n_term_phrases, int64_t* ids, int ids_ld, const int* len_ptr,
                                     float* logprob, int lp_ld, int eos, int B, int W, int V) {
    I2T_REQUIRE(lse && path_in && path_out && ids && len_ptr && logprob && (logits || (hidden && w_head)), "i2t_trie_level_expand: null pointer");
    I2T_REQUIRE(n_child >= 0 && n_term >= 0 && n_term_phrases >= 0, "i2t_trie_level_expand: n_child = %d, n_term = %d, n_term_phrases = %d: none may be negative",
                n_child, n_term, n_term_phrases);
    I2T_REQUIRE((n_child == 0 || (child_parent && child_tok)) && (n_term == 0 || (term_row && term_off && term_phrase)),
                "i2t_trie_level_expand: null pointer (a level table)");
    I2T_REQUIRE(B > 0 && W > 0 && V > 0 && ids_ld > 0 && lp_ld > 0 && (long)B * W < (1l << 31),
                "i2t_trie_level_expand: B = %d images, W = %d rows each, V = %d, ids_ld = %d, lp_ld = %d", B, W, V, ids_ld, lp_ld);
    I2T_REQUIRE(n_child <= W && n_term <= W, "i2t_trie_level_expand: n_child = %d, n_term = %d exceed the W = %d rows of an image", n_child, n_term, W);
    TRIE_TRY(check_expand_operands("i2t_trie_level_expand", hidden, ld_hidden, w_head, ld_w, d, scale, logits, ld, path_in, path_out, eos, V));
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(hidden) && ALIGNED16(w_head) && ALIGNED16(lse) && ALIGNED16(path_in) && ALIGNED16(path_out) &&
                    ALIGNED16(child_parent) && ALIGNED16(child_tok) && ALIGNED16(term_row) && ALIGNED16(term_off) && ALIGNED16(term_phrase) &&
                    ALIGNED16(ids) && ALIGNED16(logprob),
                "i2t_trie_level_expand: misaligned base pointer (16 bytes)");
    const long waves = (long)B * n_child + (long)B * n_term;
    if (waves == 0) return I2T_OK;
    I2T_REQUIRE((waves + EXPAND_WAVES - 1) / EXPAND_WAVES < (1l << 31), "i2t_trie_level_expand: %ld waves exceed a grid", waves);
    hipLaunchKernelGGL(trie_level_expand_kernel, dim3((unsigned)((waves + EXPAND_WAVES - 1) / EXPAND_WAVES)), dim3(64 * EXPAND_WAVES), 0,
                       (hipStream_t)stream, (const bf16_t*)hidden, ld_hidden, (const bf16_t*)w_head, ld_w, d, scale, logits, ld, lse, path_in,
                       path_out, child_parent, child_tok, n_child, term_row, term_off, term_phrase, n_term, n_term_phrases, ids, ids_ld, len_ptr,
                       logprob, lp_ld, eos, B, W, V);
    I2T_CHECK_LAUNCH("i2t_trie_level_expand");
    return I2T_OK;
}

// i2t_trie_level_expand with the images of one launch at different levels of different tries.  The per-image state is
// device memory, so its CONTENTS are the host's to check before upload (ops.trie_set_state); here: the operands, the sizes the kernel
// clips every image's range to, and everything i2t_trie_level_expand refuses.
extern "C" int i2t_trie_level_expand_sets(void* stream, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d, float scale,
                                          const float* logits, int ld, const float* lse, const float* path_in, float* path_out,
                                          const int* child_parent, const int* child_tok, int n_child_all, const int* term_row, int n_term_all,
                                          const int* term_off, int n_off_all, const int* term_phrase, int n_term_phrases,
                                          const int* image_state, int e_child, int e_term, int64_t* ids, int ids_ld, float* logprob, int lp_ld,
                                          int kmax, int eos, int B, int W, int V) {
    const char* fn = "i2t_trie_level_expand_sets";
    I2T_REQUIRE(lse && path_in && path_out && ids && logprob && (logits || (hidden && w_head)), "%s: null pointer", fn);
    I2T_REQUIRE(image_state, "%s: null image_state: every image names its level, its table ranges and its column", fn);
    I2T_REQUIRE(n_child_all >= 0 && n_term_all >= 0 && n_off_all >= 0 && n_term_phrases >= 0,
                "%s: n_child_all = %d, n_term_all = %d, n_off_all = %d, n_term_phrases = %d: none may be negative", fn, n_child_all, n_term_all,
                n_off_all, n_term_phrases);
    I2T_REQUIRE((n_child_all == 0 || (child_parent && child_tok)) && (n_term_all == 0 || (term_row && term_off && term_phrase)),
                "%s: null pointer (a level table)", fn);
    I2T_REQUIRE(n_term_all == 0 || n_off_all > n_term_all, "%s: n_off_all = %d offsets for n_term_all = %d terminal rows: every level has one more",
                fn, n_off_all, n_term_all);
    I2T_REQUIRE(B > 0 && W > 0 && V > 0 && ids_ld > 0 && lp_ld > 0 && (long)B * W < (1l << 31),
                "%s: B = %d images, W = %d rows each, V = %d, ids_ld = %d, lp_ld = %d", fn, B, W, V, ids_ld, lp_ld);
    I2T_REQUIRE(kmax >= 1 && kmax <= lp_ld, "%s: kmax = %d phrases per image (1 .. lp_ld = %d)", fn, kmax, lp_ld);
    I2T_REQUIRE(e_child >= 0 && e_term >= 0 && e_child <= W && e_term <= W,
                "%s: e_child = %d, e_term = %d entries per image (0 .. the W = %d rows of an image)", fn, e_child, e_term, W);
    TRIE_TRY(check_expand_operands(fn, hidden, ld_hidden, w_head, ld_w, d, scale, logits, ld, path_in, path_out, eos, V));
    I2T_REQUIRE(ALIGNED16(image_state), "%s: misaligned image_state (16 bytes)", fn);
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(hidden) && ALIGNED16(w_head) && ALIGNED16(lse) && ALIGNED16(path_in) && ALIGNED16(path_out) &&
                    ALIGNED16(child_parent) && ALIGNED16(child_tok) && ALIGNED16(term_row) && ALIGNED16(term_off) && ALIGNED16(term_phrase) &&
                    ALIGNED16(ids) && ALIGNED16(logprob),
                "%s: misaligned base pointer (16 bytes)", fn);
    const long waves = (long)B * e_child + (long)B * e_term;
    if (waves == 0) return I2T_OK;
    I2T_REQUIRE((waves + EXPAND_WAVES - 1) / EXPAND_WAVES < (1l << 31), "%s: %ld waves exceed a grid", fn, waves);
    hipLaunchKernelGGL(trie_level_expand_sets_kernel, dim3((unsigned)((waves + EXPAND_WAVES - 1) / EXPAND_WAVES)), dim3(64 * EXPAND_WAVES), 0,
                       (hipStream_t)stream, (const bf16_t*)hidden, ld_hidden, (const bf16_t*)w_head, ld_w, d, scale, logits, ld, lse, path_in,
                       path_out, child_parent, child_tok, n_child_all, term_row, n_term_all, term_off, n_off_all, term_phrase, n_term_phrases,
                       image_state, e_child, e_term, ids, ids_ld, logprob, lp_ld, kmax, eos, B, W, V);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

// ---- Beam search over the trie (search_phrases): W rows per image, each a trie node and an fp32 path sum; the N best
// phrases of the set come out of a pool of finished ones.  decoding_host.trie_beam_candidates_host / trie_beam_select_host are the
// host's statements of the two kernels.  Plain loads and vector stores, no atomics.
namespace {

constexpr int TB_MAX_W = 8;

// One workgroup per row, between the fp32 lm_head and the select kernel.  Pass A is rows_lse_kernel's -- the same helpers of
// select_common.h --, so lse is that entry point's value on the same row.  Pass B gathers the node's children: thread i takes edges
// off + i, off + i + 256, ..., total = path + (z[child_tok] - lse), and keeps its W best in registers (topk_insert); W rounds of a
// block arg-max over the threads' list heads (topk_round) give the row's W best, descending, the lower edge first on ties.
// One pass over V plus a gather over the fan-out -- no top-k over the vocabulary.  A dead row (node outside [0, nodes)) writes -1 / -inf and reads no logits.
__global__ __launch_bounds__(TRIE_THREADS) void trie_beam_candidates_kernel(const float* __restrict__ logits, int ld, const int* __restrict__ node,
                                                                            const float* __restrict__ path, const int* __restrict__ child_off,
                                                                            const int* __restrict__ child_tok, const int* __restrict__ term,
                                                                            int nodes, int edges, int eos, const int* __restrict__ ctrl,
                                                                            int* __restrict__ cand_edge, float* __restrict__ cand_total,
                                                                            float* __restrict__ fin_total, float* __restrict__ lse_out, int W, int V) {
    __shared__ float rmx[TRIE_THREADS / 64], rse[TRIE_THREADS / 64], sh_v[TRIE_THREADS / 64], sh_lse;
    __shared__ int sh_e[TRIE_THREADS / 64], sh_win;
    if (ctrl[0]) return;                                // block-uniform, before any barrier
    const int r = blockIdx.x, tid = threadIdx.x;
    const int nd = node[r];
    if (nd < 0 || nd >= nodes) {                        // block-uniform
        if (tid < W) {
            cand_edge[(size_t)r * W + tid] = -1;
            cand_total[(size_t)r * W + tid] = -INFINITY;
        }
        if (tid == 0) fin_total[r] = -INFINITY;
        return;
    }
    const float* z = logits + (size_t)r * ld;
    float mx, se;
    row_lse_partials<TRIE_THREADS>(z, V, mx, se, rmx, rse);
    __syncthreads();
    if (tid == 0) sh_lse = lse_waves_merge<TRIE_THREADS>(mx, se, rmx, rse);
    __syncthreads();
    const float lse = sh_lse, p = path[r];
    if (tid == 0) {
        if (lse_out) lse_out[r] = lse;
        fin_total[r] = term[nd] >= 0 ? p + (z[eos] - lse) : -INFINITY;
    }
    int off, fan;
    node_edges(child_off, nd, edges, edges, off, fan);
    float kv[TB_MAX_W];
    int ke[TB_MAX_W];
    topk_clear(kv, ke);
    for (int i = tid; i < fan; i += TRIE_THREADS) {
        const int t = child_tok[off + i];
        topk_insert(kv, ke, W, p + (((t >= 0 && t < V) ? z[t] : -INFINITY) - lse), off + i);
    }
    for (int j = 0; j < W; ++j)
        topk_round<TRIE_THREADS>(kv, ke, sh_v, sh_e, &sh_win, [&](float bv, int be) {
            cand_edge[(size_t)r * W + j] = be == TOPK_NONE ? -1 : be;
            cand_total[(size_t)r * W + j] = be == TOPK_NONE ? -INFINITY : bv;
        });
}

// One workgroup per image, after the candidates kernel.  Thread 0 does the bookkeeping in the replica's order: the rows' offers into
// the pool (an entry held before a new one of equal score), the W best of the rows' sorted candidate lists by a W-way merge (the lower
// row first on ties; within a row the list's order), the close test.  Then every thread moves history columns [0, pos) from the W
// parents to the W children (select_common.h's move_rows: every parent column is read before a child row is written),
// and threads 0 .. W - 1 write the children's node, path, token and hist[child][pos] = parent.  A row without a child is dead: node
// -1, path -inf, token eos, its own history row.  Every open image stores the same 1 into ctrl[1]: no atomic.
// SETS (i2t_trie_beam_select_sets): image b has its own prompt length plen[b] (plen null: P) and its own longest phrase
// longest_of[b].  With t = len - plen[b] < 0 the image sits in a forced prompt column: pool, node, path, closed and ids stay, every row
// records itself as its parent at hist[row][pos], and the image stores the 1 into ctrl[1] that keeps the search open.
constexpr int TS_THREADS = 256;
template <bool SETS>
__global__ __launch_bounds__(TS_THREADS) void trie_beam_select_kernel(const int* __restrict__ cand_edge, const float* __restrict__ cand_total,
                                                                      const float* __restrict__ fin_total, int* __restrict__ node,
                                                                      float* __restrict__ path, const int* __restrict__ child_tok,
                                                                      const int* __restrict__ child_next, const int* __restrict__ term, int nodes,
                                                                      int edges, int eos, int64_t* __restrict__ ids, int ids_ld, int* hist,
                                                                      int hist_ld, int* __restrict__ pool_phrase, float* __restrict__ pool_sum,
                                                                      float* __restrict__ pool_score, int* __restrict__ pool_len,
                                                                      int* __restrict__ pool_n, int* __restrict__ closed,
                                                                      const int* __restrict__ pos_ptr, const int* __restrict__ len_ptr,
                                                                      int* __restrict__ ctrl, int W, int P, int longest_all, float length_penalty,
                                                                      const int* __restrict__ plen, const int* __restrict__ longest_of) {
    __shared__ int c_par[TB_MAX_W], c_node[TB_MAX_W], c_tok[TB_MAX_W], head[TB_MAX_W];
    __shared__ float c_path[TB_MAX_W];
    __shared__ int e_ph[TB_MAX_W + 1], e_len[TB_MAX_W + 1];
    __shared__ float e_score[TB_MAX_W + 1], e_sum[TB_MAX_W + 1];
    if (ctrl[0]) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (closed[b]) return;
    const int longest = SETS ? longest_of[b] : longest_all;
    const int pos = *pos_ptr, len = *len_ptr, t = len - ((SETS && plen) ? plen[b] : P);
    const int r0 = b * W;
    if (SETS && t < 0) {                                // block-uniform: a forced column
        if (len < 0 || pos < 0 || pos >= hist_ld) return;
        if (tid < W) hist[(size_t)(r0 + tid) * hist_ld + pos] = r0 + tid;
        if (tid == 0) ctrl[1] = 1;
        return;
    }
    if (t < 0 || t > longest || len >= ids_ld || pos < 0 || pos >= hist_ld) return;      // counters outside the call's columns: nothing is written
    if (tid == 0) {
        int m = pool_n[b];
        m = m < 0 ? 0 : (m > W ? W : m);
        for (int i = 0; i < m; ++i) {
            e_score[i] = pool_score[r0 + i];
            e_sum[i] = pool_sum[r0 + i];
            e_ph[i] = pool_phrase[r0 + i];
            e_len[i] = pool_len[r0 + i];
        }
        const float denom = powf((float)(t + 1), length_penalty);
        for (int w = 0; w < W; ++w) {
            const int nd = node[r0 + w];
            head[w] = (nd >= 0 && nd < nodes) ? 0 : W;       // a dead row has no list
            if (nd < 0 || nd >= nodes || term[nd] < 0) continue;
            const float f = fin_total[r0 + w], s = f / denom;
            int at = 0;
            while (at < m && e_score[at] >= s) ++at;         // behind everything at least as good
            if (at >= W) continue;
            for (int i = (m < W ? m : W - 1); i > at; --i) {
                e_score[i] = e_score[i - 1];
                e_sum[i] = e_sum[i - 1];
                e_ph[i] = e_ph[i - 1];
                e_len[i] = e_len[i - 1];
            }
            e_score[at] = s;
            e_sum[at] = f;
            e_ph[at] = term[nd];
            e_len[at] = t + 1;
            if (m < W) ++m;
        }
        int nchild = 0;
        for (int k = 0; k < W; ++k) {
            int bw = -1, be = -1;
            float bv = 0.f;
            for (int w = 0; w < W; ++w) {
                if (head[w] >= W) continue;
                const int e = cand_edge[(size_t)(r0 + w) * W + head[w]];
                if (e < 0 || e >= edges) {                   // the row's list ends here
                    head[w] = W;
                    continue;
                }
                const float v = cand_total[(size_t)(r0 + w) * W + head[w]];
                if (bw < 0 || v > bv) {
                    bw = w;
                    be = e;
                    bv = v;
                }
            }
            if (bw < 0) break;
            c_par[k] = r0 + bw;
            c_node[k] = child_next[be];
            c_tok[k] = child_tok[be];
            c_path[k] = bv;
            ++head[bw];
            ++nchild;
        }
        for (int k = nchild; k < W; ++k) {
            c_par[k] = r0 + k;
            c_node[k] = -1;
            c_tok[k] = eos;
            c_path[k] = -INFINITY;
        }
        int cl = nchild == 0 ? 1 : 0;
        if (!cl && m == W) {
            const float lopt = powf((float)(length_penalty >= 0.f ? longest + 1 : t + 2), length_penalty);
            cl = c_path[0] / lopt > e_score[W - 1] ? 0 : 1;
        }
        for (int i = 0; i < m; ++i) {
            pool_score[r0 + i] = e_score[i];
            pool_sum[r0 + i] = e_sum[i];
            pool_phrase[r0 + i] = e_ph[i];
            pool_len[r0 + i] = e_len[i];
        }
        pool_n[b] = m;
        closed[b] = cl;
        if (!cl) ctrl[1] = 1;
    }
    __syncthreads();
    move_rows<TB_MAX_W>(hist, hist_ld, c_par, r0, W, pos, TS_THREADS);
    if (tid < W) {
        const int c = r0 + tid;
        node[c] = c_node[tid];
        path[c] = c_path[tid];
        ids[(size_t)c * ids_ld + len] = c_tok[tid];
        hist[(size_t)c * hist_ld + pos] = c_par[tid];
    }
}

// The checks and the launch i2t_trie_beam_select and i2t_trie_beam_select_sets share; `fn` names the caller in every message.
// longest_of null: the plain kernel, one prompt length P and one longest phrase for every image, both held against ids_ld here.
int trie_select_launch(const char* fn, void* stream, const int* cand_edge, const float* cand_total, const float* fin_total, int* node,
                       float* path, const int* child_tok, const int* child_next, const int* term, int nodes, int edges, int eos, int64_t* ids,
                       int ids_ld, int* hist, int hist_ld, int* pool_phrase, float* pool_sum, float* pool_score, int* pool_len, int* pool_n,
                       int* closed, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int P, int longest, float length_penalty,
                       const int* plen, const int* longest_of) {
    I2T_REQUIRE(cand_edge && cand_total && fin_total && node && path && child_tok && child_next && term && ids && hist && pool_phrase &&
                    pool_sum && pool_score && pool_len && pool_n && closed && pos_ptr && len_ptr && ctrl,
                "%s: null pointer", fn);
    I2T_REQUIRE(B > 0 && (long)B * TB_MAX_W < (1l << 31), "%s: B = %d images", fn, B);
    I2T_REQUIRE(W >= 1 && W <= TB_MAX_W, "%s: W = %d rows per image (1 .. %d)", fn, W, TB_MAX_W);
    if (longest_of) {
        I2T_REQUIRE(P >= 1, "%s: P = %d (at least 1)", fn, P);
        I2T_REQUIRE((long)P + 2 <= ids_ld && hist_ld >= 1, "%s: P + 2 = %ld columns exceed ids_ld = %d (hist_ld = %d)", fn, (long)P + 2, ids_ld,
                    hist_ld);
    } else {
        I2T_REQUIRE(P >= 1 && longest >= 1, "%s: P = %d, longest = %d (each at least 1)", fn, P, longest);
        I2T_REQUIRE((long)P + longest + 1 <= ids_ld && hist_ld >= 1, "%s: P + longest + 1 = %ld columns exceed ids_ld = %d (hist_ld = %d)", fn,
                    (long)P + longest + 1, ids_ld, hist_ld);
    }
    TRIE_TRY(check_trie_tables(fn, nodes, edges));
    I2T_REQUIRE(eos >= 0, "%s: eos = %d: a dead row takes it as its token", fn, eos);
    // the exponent bits, not a comparison: no fast-math folding of a NaN test
    I2T_REQUIRE((__builtin_bit_cast(unsigned, length_penalty) & 0x7f800000u) != 0x7f800000u, "%s: length_penalty must be finite", fn);
    if (longest_of)
        hipLaunchKernelGGL(trie_beam_select_kernel<true>, dim3(B), dim3(TS_THREADS), 0, (hipStream_t)stream, cand_edge, cand_total, fin_total, node,
                           path, child_tok, child_next, term, nodes, edges, eos, ids, ids_ld, hist, hist_ld, pool_phrase, pool_sum, pool_score,
                           pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, W, P, 0, length_penalty, plen, longest_of);
    else
        hipLaunchKernelGGL(trie_beam_select_kernel<false>, dim3(B), dim3(TS_THREADS), 0, (hipStream_t)stream, cand_edge, cand_total, fin_total, node,
                           path, child_tok, child_next, term, nodes, edges, eos, ids, ids_ld, hist, hist_ld, pool_phrase, pool_sum, pool_score,
                           pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, W, P, longest, length_penalty, nullptr, nullptr);
    I2T_CHECK_LAUNCH(fn);
    return I2T_OK;
}

}  // namespace

extern "C" int i2t_trie_beam_candidates(void* stream, const float* logits, int ld, const int* node, const float* path, const int* child_off,
                                        const int* child_tok, const int* term, int nodes, int edges, int eos, const int* ctrl, int* cand_edge,
                                        float* cand_total, float* fin_total, float* lse, int R, int W, int V) {
    I2T_REQUIRE(logits && node && path && child_off && child_tok && term && ctrl && cand_edge && cand_total && fin_total,
                "i2t_trie_beam_candidates: null pointer");
    I2T_REQUIRE(R > 0 && V > 0, "i2t_trie_beam_candidates: R = %d rows, V = %d", R, V);
    I2T_REQUIRE(W >= 1 && W <= TB_MAX_W, "i2t_trie_beam_candidates: W = %d candidates per row (1 .. %d)", W, TB_MAX_W);
    TRIE_TRY(check_logits_rows("i2t_trie_beam_candidates", ld, V));
    TRIE_TRY(check_eos_in_vocab("i2t_trie_beam_candidates", eos, V));
    TRIE_TRY(check_trie_tables("i2t_trie_beam_candidates", nodes, edges));
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(node) && ALIGNED16(path) && ALIGNED16(child_off) && ALIGNED16(child_tok) && ALIGNED16(term) &&
                    ALIGNED16(cand_edge) && ALIGNED16(cand_total) && ALIGNED16(fin_total) && ALIGNED16(lse),
                "i2t_trie_beam_candidates: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(trie_beam_candidates_kernel, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, node, path, child_off,
                       child_tok, term, nodes, edges, eos, ctrl, cand_edge, cand_total, fin_total, lse, W, V);
    I2T_CHECK_LAUNCH("i2t_trie_beam_candidates");
    return I2T_OK;
}

extern "C" int i2t_trie_beam_select(void* stream, const int* cand_edge, const float* cand_total, const float* fin_total, int* node, float* path,
                                    const int* child_tok, const int* child_next, const int* term, int nodes, int edges, int eos, int64_t* ids,
                                    int ids_ld, int* hist, int hist_ld, int* pool_phrase, float* pool_sum, float* pool_score, int* pool_len,
                                    int* pool_n, int* closed, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int P,
                                    int longest, float length_penalty) {
    return trie_select_launch("i2t_trie_beam_select", stream, cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, nodes,
                              edges, eos, ids, ids_ld, hist, hist_ld, pool_phrase, pool_sum, pool_score, pool_len, pool_n, closed, pos_ptr, len_ptr,
                              ctrl, B, W, P, longest, length_penalty, nullptr, nullptr);
}

// i2t_trie_beam_select with a prompt length and a longest phrase per image, both device tables.  The host cannot hold
// the tables against ids_ld; the kernel writes no id column at or past ids_ld and no history column outside [0, hist_ld).
extern "C" int i2t_trie_beam_select_sets(void* stream, const int* cand_edge, const float* cand_total, const float* fin_total, int* node,
                                         float* path, const int* child_tok, const int* child_next, const int* term, int nodes, int edges, int eos,
                                         int64_t* ids, int ids_ld, int* hist, int hist_ld, int* pool_phrase, float* pool_sum, float* pool_score,
                                         int* pool_len, int* pool_n, int* closed, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W,
                                         int P, const int* plen, const int* longest_of, float length_penalty) {
    I2T_REQUIRE(longest_of, "i2t_trie_beam_select_sets: null longest_of: every image names its set's longest phrase");
    I2T_REQUIRE(ALIGNED16(plen) && ALIGNED16(longest_of), "i2t_trie_beam_select_sets: misaligned plen or longest_of (16 bytes)");
    return trie_select_launch("i2t_trie_beam_select_sets", stream, cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, nodes,
                              edges, eos, ids, ids_ld, hist, hist_ld, pool_phrase, pool_sum, pool_score, pool_len, pool_n, closed, pos_ptr,
                              len_ptr, ctrl, B, W, P, 0, length_penalty, plen, longest_of);
}
