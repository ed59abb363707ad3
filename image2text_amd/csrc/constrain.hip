// Closed-set decoding of generate_captions(phrases=...): a pre-pass and a post-pass around the fp32-logits choosers of a
// caption step, which run between them as they are.  The phrase set is a flat CSR trie in device memory (decoding.phrase_trie): the
// children of node n are edges child_off[n] .. child_off[n + 1), child_tok ascending, child_next the node an edge leads to, term[n] the
// index of the phrase that ends at n or -1; node 0 is the root.  Every row keeps its node in node[r].  Plain loads and vector stores,
// no atomics; nothing is read or written once *done is set.
#include "common.h"

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

// The pre-pass, between the lm_head GEMM and the chooser: one workgroup per row.  Pass A: the RAW row's (max, sum exp) -- a thread's
// chain, a fixed xor tree, the waves in order (caption_logits_process_kernel's shape: bit-reproducible) -> raw_lse[r]; in the same pass
// kept[r][i] = z[child_tok[off + i]] for the node's children and kept[r][fan] = z[eos] at a terminal node, all raw since nothing has
// been written.  Barrier.  Pass B: -inf over columns [0, V), 16-byte stores; columns V .. ld are not touched.  Barrier.  Pass C: the
// kept values back into their columns (thread i of pass A wrote kept[r][i] and reads it here itself).  Any fan-out works: no LDS bitmap,
// no limit on V.  decoding.trie_mask_host is the host's statement of what the row holds afterwards.
constexpr int TRIE_THREADS = 256;
__global__ __launch_bounds__(TRIE_THREADS) void caption_trie_mask_kernel(float* logits, int ld, const int* __restrict__ node,
                                                                         const int* __restrict__ child_off, const int* __restrict__ child_tok,
                                                                         const int* __restrict__ term, int nodes, int edges, int eos,
                                                                         const int* __restrict__ done, float* __restrict__ raw_lse, float* kept,
                                                                         int kept_ld, int V) {
    __shared__ float rmx[TRIE_THREADS / 64], rse[TRIE_THREADS / 64];
    if (*done) return;                                  // block-uniform, before any barrier
    const int r = blockIdx.x, tid = threadIdx.x;
    const int nd = node[r];
    if (nd < 0 || nd >= nodes) return;                  // block-uniform (never from the advance kernel)
    int off, fan;
    node_edges(child_off, nd, edges, kept_ld - 1, off, fan);
    const bool terminal = term[nd] >= 0;
    float* z = logits + (size_t)r * ld;
    float* kp = kept + (size_t)r * kept_ld;
    float mx = -INFINITY, se = 0.f;
    const int vend = V & ~3;                            // (ld % 4 == 0 and a 16-byte base: the entry point's checks)
    for (int c4 = tid * 4; c4 < vend; c4 += TRIE_THREADS * 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(z + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) lse_add(mx, se, q[e]);
    }
    for (int c = vend + tid; c < V; c += TRIE_THREADS) lse_add(mx, se, z[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(mx, se, __shfl_xor(mx, o, 64), __shfl_xor(se, o, 64));
    if ((tid & 63) == 0) {
        rmx[tid >> 6] = mx;
        rse[tid >> 6] = se;
    }
    for (int i = tid; i < fan; i += TRIE_THREADS) {
        const int t = child_tok[off + i];
        kp[i] = (t >= 0 && t < V) ? z[t] : -INFINITY;
    }
    if (tid == 0 && terminal) kp[fan] = z[eos];
    __syncthreads();                                    // every read of the raw row is done
    if (tid == 0) {
        for (int k = 1; k < TRIE_THREADS / 64; ++k) lse_merge(mx, se, rmx[k], rse[k]);
        raw_lse[r] = mx + logf(se);
    }
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
constexpr int TRIE_ADV_WAVES = 4;
__global__ __launch_bounds__(64 * TRIE_ADV_WAVES) void caption_trie_advance_kernel(const int64_t* __restrict__ ids, int ids_ld,
                                                                                   const int* __restrict__ len_ptr, const int* __restrict__ finished,
                                                                                   const float* __restrict__ logits, int ld,
                                                                                   const float* __restrict__ raw_lse, const int* __restrict__ child_off,
                                                                                   const int* __restrict__ child_tok, const int* __restrict__ child_next,
                                                                                   const int* __restrict__ term, int nodes, int edges, int eos,
                                                                                   const int* __restrict__ done, int* __restrict__ node,
                                                                                   int* __restrict__ phrase_index, float* __restrict__ tok_lp, int lp_ld,
                                                                                   int R, int V) {
    if (*done) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * TRIE_ADV_WAVES + (threadIdx.x >> 6);
    const int len = *len_ptr;
    if (r >= R || len < 0 || len >= ids_ld || len >= lp_ld) return;      // wave-uniform, as every return below
    if (finished[r]) return;
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

}  // namespace

extern "C" int i2t_caption_trie_mask(void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                                     const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept, int kept_ld,
                                     int R, int V) {
    I2T_REQUIRE(logits && node && child_off && child_tok && term && done && raw_lse && kept, "i2t_caption_trie_mask: null pointer");
    I2T_REQUIRE(R > 0 && V > 0, "i2t_caption_trie_mask: R = %d rows, V = %d", R, V);
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "i2t_caption_trie_mask: ld = %d: logits rows hold V = %d columns and start on 16 bytes", ld, V);
    I2T_REQUIRE(eos >= 0 && eos < V, "i2t_caption_trie_mask: eos = %d outside the vocabulary of %d", eos, V);
    I2T_REQUIRE(nodes >= 1 && edges >= 0, "i2t_caption_trie_mask: nodes = %d, edges = %d: a trie has a root", nodes, edges);
    I2T_REQUIRE(kept_ld >= 1, "i2t_caption_trie_mask: kept_ld = %d: a row keeps at least the EOS logit", kept_ld);
    I2T_REQUIRE(ALIGNED16(logits) && ALIGNED16(kept) && ALIGNED16(raw_lse) && ALIGNED16(node) && ALIGNED16(child_off) && ALIGNED16(child_tok) &&
                    ALIGNED16(term),
                "i2t_caption_trie_mask: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(caption_trie_mask_kernel, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, node, child_off, child_tok, term,
                       nodes, edges, eos, done, raw_lse, kept, kept_ld, V);
    I2T_CHECK_LAUNCH("i2t_caption_trie_mask");
    return I2T_OK;
}

extern "C" int i2t_caption_trie_advance(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                                        const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok,
                                        const int* child_next, const int* term, int nodes, int edges, int eos, const int* done, int* node,
                                        int* phrase_index, float* tok_lp, int lp_ld, int R, int V) {
    I2T_REQUIRE(ids && len_ptr && finished && logits && raw_lse && child_off && child_tok && child_next && term && done && node && phrase_index &&
                    tok_lp,
                "i2t_caption_trie_advance: null pointer");
    I2T_REQUIRE(R > 0 && V > 0 && ids_ld > 0 && lp_ld > 0, "i2t_caption_trie_advance: R = %d rows, V = %d, ids_ld = %d, lp_ld = %d", R, V, ids_ld,
                lp_ld);
    I2T_REQUIRE(ld >= V && ld % 4 == 0, "i2t_caption_trie_advance: ld = %d: logits rows hold V = %d columns and start on 16 bytes", ld, V);
    I2T_REQUIRE(eos >= 0 && eos < V, "i2t_caption_trie_advance: eos = %d outside the vocabulary of %d", eos, V);
    I2T_REQUIRE(nodes >= 1 && edges >= 0, "i2t_caption_trie_advance: nodes = %d, edges = %d: a trie has a root", nodes, edges);
    I2T_REQUIRE(ALIGNED16(ids) && ALIGNED16(logits) && ALIGNED16(raw_lse) && ALIGNED16(node) && ALIGNED16(phrase_index) && ALIGNED16(child_off) &&
                    ALIGNED16(child_tok) && ALIGNED16(child_next) && ALIGNED16(term),
                "i2t_caption_trie_advance: misaligned base pointer (16 bytes)");
    hipLaunchKernelGGL(caption_trie_advance_kernel, dim3((R + TRIE_ADV_WAVES - 1) / TRIE_ADV_WAVES), dim3(64 * TRIE_ADV_WAVES), 0,
                       (hipStream_t)stream, ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok, child_next, term, nodes,
                       edges, eos, done, node, phrase_index, tok_lp, lp_ld, R, V);
    I2T_CHECK_LAUNCH("i2t_caption_trie_advance");
    return I2T_OK;
}
