// Which kernel an i2t_gemm_bf16 call reaches: the whole decision, as plain C++17 on plain values (no HIP, no pointer is read), so that
// it runs on a CPU -- tests/test_gemm_route_cpu.py holds a table of calls and the routes they must take.  gemm.hip validates the
// arguments, describes the call as a GemmCall, reads the environment into GemmKnobs, asks gemm_route() and launches what it says.
//
// The rule, top to bottom (the first that applies):
//   1. skinny      M <= 64, both operands row-major, at most bias / GELU / residual: the weight-streaming kernel;
//   2. dW          both operands k-major, plain accumulate into an fp32 C of >= 256 x 256: the 256^2 kernel over K chunks that fit a
//                  32-bit buffer offset, each chunk as one slice (class 5) or as K slices with atomics (class 6, or 13 with the column
//                  sum folded in).  A first chunk with no such form sends the call on down this list; a later one is an error;
//   3. gemm3       only when I2T_GEMM3 asks for it;
//   4. 256^2       >= I2T_G256_MIN_TILES (40) tiles, N > 128, A row-major, K % 128 == 0 or B k-major: persistent, by epilogue class;
//   5. 128^2       everything else, split-K for plain accumulates with too few tiles.
#pragma once
#include "../../include/i2t.h"

namespace i2t {

// One i2t_gemm_bf16 call, as far as routing reads it.  Pointers appear only as the facts taken from them.
struct GemmCall {
    int M, N, K;
    int lda, ldb, ldc;
    bool a_kmajor, b_kmajor;
    int c_is_f32, accumulate, act, drop_mode;
    bool bias, aux_in, aux_out, residual;     // present?
    int ld_aux_in, ld_aux_out, ldr;
    bool alpha_one, alpha_sumsq;              // alpha == 1.0f; the gradient normaliser is present
    bool colsum_out;                          // i2t_gemm_dw_colsum_bf16: the A panel's row sums are wanted as well
    bool c_aligned16, aux_out_aligned16;      // 16-byte alignment of C and aux_out (gemm3's stores)
    bool residual_is_c;                       // residual == C (the skinny kernel's in-place residual form)
};

// One field per I2T_* variable the GEMM host code reads (gemm.hip::gemm_knobs fills it).
struct GemmKnobs {
    bool no_g256;            // I2T_GEMM=v1: every GEMM on the 128^2 kernel
    long min_tiles;          // I2T_G256_MIN_TILES: tile count from which the large-tile kernel takes over (40)
    int gemm3;               // I2T_GEMM3 = 0 never | 1 always, epilogue after the K loop | 2 always, overlapped | unset (0): the default rule
    bool narrow_256;         // I2T_G256_NARROW=1: N <= 128 on the 256^2 kernel as well (the old routing, for A/B)
    bool skinny_ksplit;      // I2T_SKINNY_KSPLIT set: the skinny kernel may split K across workgroups
    bool fold_colsum;        // I2T_FOLD_COLSUM != 0: the bias gradient inside the split-K dW kernel
    int dw_splits;           // I2T_DW_SPLITS: K slices of a split dW (experiments); 0: n_cu / tiles
    int gn;                  // I2T_G256_GN: column tiles per group of the 256^2 tile order (8)
    int stagger, stagger_groups;   // I2T_G256_STAGGER = "units[,groups]"
    int g256_dbg;            // I2T_G256_DBG
    int g3_dbg;              // I2T_G3_DBG
    bool fp8_g256;           // I2T_FP8_G256 != 0: fp8 operands may take the 256^2 kernel
    bool log;                // I2T_GEMM_LOG set
};

// Epilogue class of the 256^2 kernel (and of gemm3) for this call; 0 = the generic one.
inline int g256_epilogue_class(const GemmCall& p) {
    const bool fast4 = (p.ldc & 3) == 0 && (!p.residual || (p.ldr & 3) == 0) && (!p.aux_in || (p.ld_aux_in & 3) == 0) &&
                       (!p.aux_out || (p.ld_aux_out & 3) == 0);
    const bool none = p.act == I2T_ACT_NONE && !p.aux_out;
    // bias-free only: a straddling quad would read bias[N .. N+2]
    if (fast4 && (p.N & 3) != 0 && none && !p.bias && !p.residual && !p.accumulate && !p.drop_mode) return 7;
    if (!fast4 || (p.N & 3) != 0) return 0;
    if (!p.c_is_f32 && none && !p.residual && !p.accumulate && p.drop_mode != 1) return 1;
    if (!p.c_is_f32 && p.act == I2T_ACT_GELU && !p.drop_mode && !p.residual && !p.accumulate) return 2;
    if (!p.c_is_f32 && p.act == I2T_ACT_GELU_DOUT && !p.drop_mode && !p.residual && !p.accumulate) return 10;
    if (!p.c_is_f32 && p.act == I2T_ACT_MUL_AUX && !p.bias && !p.aux_out && !p.drop_mode && !p.residual && !p.accumulate) return 11;
    if (p.c_is_f32 && none && !p.accumulate && p.drop_mode != 2 && (p.residual || p.bias || p.drop_mode)) return 3;
    if (!p.c_is_f32 && p.act == I2T_ACT_DGELU && !p.bias && !p.aux_out && !p.drop_mode && !p.residual && !p.accumulate) return 4;
    if (p.c_is_f32 && none && !p.bias && !p.residual && !p.drop_mode) return 5;
    return 0;
}

enum class Colsum { None, Folded, Before };     // the column sum: absent | inside the split-K dW kernel (class 13) | a colsum_kernel launch ahead of the GEMM

// How one K chunk of a dW GEMM runs on the 256^2 kernel.  cls 0: it has no large-tile form.
struct DwPlan {
    int cls;                 // 5: one K slice, plain read-add-write epilogue | 6: K slices + float atomics | 13: 6 with the column sum folded in
    int splits, per;         // K slices per output tile and K-tiles per slice (even)
    Colsum colsum;
};

// dW = A^T . B accumulated into an fp32 C (both operands k-major): K slices spread over the CUs when the output has too
// few 256^2 tiles, partial tiles combined with float atomics (C already holds the value to accumulate onto); with enough
// tiles (the tied lm_head / embedding gradient) one slice and a plain read-add-write epilogue.
// colsum_out: the row sums of the A panel are added to it as well -- inside the split-K kernel (class 13) unless
// I2T_FOLD_COLSUM=0, by a column-sum launch of their own next to the one-slice form.
inline DwPlan dw_plan(int M, int N, int Kchunk, bool class5, bool colsum_out, const GemmKnobs& knobs, int n_cu, bool deterministic) {
    const int tiles = ((M + 255) / 256) * ((N + 255) / 256), nk_all = (Kchunk + 63) >> 6;
    const Colsum own_launch = colsum_out ? Colsum::Before : Colsum::None;
    if (tiles >= n_cu || n_cu / tiles < 2 || deterministic) {      // (deterministic mode: one K slice, no atomics)
        // (more than half a round of tiles but less than one -- a Qwen2-1.5B down_proj dW, 1536 x 8960 = 210 tiles -- cannot be split:
        // one tile per workgroup on the persistent kernel still beats the 128^2 fallback it used to take, 711 TF)
        if (!class5) return DwPlan{0, 0, 0, Colsum::None};
        return DwPlan{5, 1, (nk_all + 1) & ~1, own_launch};
    }
    int splits = knobs.dw_splits ? knobs.dw_splits : n_cu / tiles;
    int per = ((nk_all + splits - 1) / splits + 1) & ~1;          // even number of K-tiles per slice
    if (per < 8) per = 8;
    splits = (nk_all + per - 1) / per;
    if (splits < 2) return DwPlan{0, 0, 0, Colsum::None};
    if (colsum_out && knobs.fold_colsum) return DwPlan{13, splits, per, Colsum::Folded};
    return DwPlan{6, splits, per, own_launch};
}

enum class RouteKind { Skinny, DW, Gemm3, G256, G128 };

struct GemmRoute {
    RouteKind kind;
    int mt, ksplit;          // Skinny: 16-row subtiles (1 .. 4) and K slices across workgroups
    int cls;                 // G256, Gemm3: epilogue class, 0 where the class is not built for the layout
    bool overlap;            // Gemm3: the previous tile's epilogue inside the K loop
    long kc;                 // DW: chunk length; chunk i covers K rows [i kc, min(K, (i + 1) kc))
    int chunks;              // DW: chunks to launch, from the first
    bool chunk_error;        // DW: the chunk after those has no large-tile form: the call fails there
    DwPlan full, tail;       // DW: plan of the chunks of length kc and of a shorter last one
    int splits;              // G128: K slices (1: the fused epilogue; > 1: float atomics onto C)
    Colsum colsum;           // every kind but DW (whose plans carry it): Before when the call wants the column sum, else None
};

inline GemmRoute gemm_route(const GemmCall& c, const GemmKnobs& knobs, int n_cu, bool deterministic) {
    GemmRoute r{};
    if (c.M <= 64 && !c.a_kmajor && !c.b_kmajor && !c.aux_out && c.act <= I2T_ACT_GELU && !c.accumulate && !c.drop_mode) {
        // decode-step shape: weight-streaming kernel.  In-place residual form (C is fp32 and IS the residual) may also
        // split K across workgroups when there are too few column tiles to pull HBM bandwidth from every CU.
        r.kind = RouteKind::Skinny;
        r.ksplit = 1;
        const int ntiles = (c.N + 15) / 16;
        // NOTE: the cross-workgroup split is OFF by default: float atomics make the sum order, hence the last bits of
        // the logits, vary from run to run, and greedy decoding must be token-exact reproducible.  The N = 768
        // projections then run on 48 workgroups; they are launch-latency-sized anyway (1.2 - 4.7 MB of weights).
        if (knobs.skinny_ksplit && c.c_is_f32 && c.residual_is_c && c.ldr == c.ldc && c.act == I2T_ACT_NONE && !c.accumulate)
            while (ntiles * r.ksplit < 256 && (c.K / 64) / (r.ksplit * 2) >= 2 && r.ksplit < 16) r.ksplit *= 2;
        const int mt = (c.M + 15) / 16;
        r.mt = mt < 4 ? mt : 4;
        return r;
    }
    if (!knobs.no_g256 && c.a_kmajor && c.b_kmajor && c.accumulate && c.c_is_f32 && !c.bias && c.act == I2T_ACT_NONE && !c.aux_out && !c.residual &&
        !c.drop_mode && c.M >= 256 && c.N >= 256 && (c.ldc & 3) == 0 && (c.N & 3) == 0) {
        // The k-major panels are addressed through 32-bit buffer offsets: (K + 512) rows x ld x 2 bytes must stay below 4 GiB.
        // A longer reduction (B = 2048: the tied lm_head's dW reads 74 k rows of 50 264 logits, the projector's 401 k rows of
        // 8192) runs as consecutive K chunks that accumulate into the same C -- it used to fall back to the 128^2 kernel
        // (731 / 789 TF instead of ~1.1 / 1.3 PF).
        const unsigned long long ld_max = (unsigned long long)(c.lda > c.ldb ? c.lda : c.ldb);
        const long k_fit = (long)((1ull << 32) / (2 * ld_max)) - 512;
        if (k_fit >= 1024) {
            const bool class5 = g256_epilogue_class(c) == 5;
            r.kc = (c.K <= k_fit) ? c.K : (k_fit / 128) * 128;
            const int n_full = (int)(c.K / r.kc), k_tail = (int)(c.K - n_full * r.kc);
            r.full = dw_plan(c.M, c.N, (int)r.kc, class5, c.colsum_out, knobs, n_cu, deterministic);
            // a first chunk with no large-tile form: the call takes the 128^2 route below; a later one (only a short tail can differ
            // from the first) is an error, reported after the chunks before it have run
            if (r.full.cls) {
                r.kind = RouteKind::DW;
                r.chunks = n_full;
                if (k_tail) {
                    r.tail = dw_plan(c.M, c.N, k_tail, class5, c.colsum_out, knobs, n_cu, deterministic);
                    if (r.tail.cls) ++r.chunks;
                    else r.chunk_error = true;
                }
                return r;
            }
            r = GemmRoute{};
        }
    }
    r.colsum = c.colsum_out ? Colsum::Before : Colsum::None;      // (no large-tile split-K form for this call: its own launch)
    // split-K for accumulate-into-fp32 problems whose tile grid cannot fill the 256 CUs (the dW = dY^T.X GEMMs: small
    // M x N, very long K): enough slices to reach ~2 workgroups per CU, each slice at least 4 K-steps long
    int splits = 1;
    const bool plain_epilogue = !c.bias && c.act == I2T_ACT_NONE && !c.aux_out && !c.residual && !c.drop_mode;
    if (c.accumulate && c.c_is_f32 && plain_epilogue) {
        const int tiles = ((c.M + 127) / 128) * ((c.N + 127) / 128), nk_all = (c.K + 63) / 64;
        while (tiles * splits < 384 && nk_all / (splits * 2) >= 4 && splits < 64) splits *= 2;
        if (deterministic) splits = 1;            // deterministic mode: one K slice per tile, plain read-add-write epilogue
    }
    // gemm3 (256 x 128 tiles, the previous tile's epilogue inside the K loop): bit-equal to the 256^2 kernel; measured on MI355X
    // (tools/bench_gemm3.py) +8.5 % at K = 512 (class 1: 865 vs 797 TF), a tie at K = 768 (993 vs 979, 963 vs 953, 1026 vs 1058)
    // and -14 % at K = 2048 (its K loop moves 1.33x the LDS bytes per MFMA and is LDS-bound); the GELU class LOSES (458 vs 704 TF:
    // a 64-value GELU step per wave outlasts the MFMA block it is meant to hide behind).  Default: class 1 with K <= 512 only ...
    // I2T_GEMM3 = 0 never | 1 always, epilogue after the K loop | 2 always, overlapped | unset: the default rule.
    // ... and only without the per-row dropout multipliers and up to ~4e5 rows: at the benchmark's M = 798 720 (B = 3072) the
    // 256^2 kernel is the faster one (1363 vs 1654 us with dropout, 1417 vs 1528 without), and with dropout gemm3 does not win
    // at M = 266 240 either (515 vs 513 us)
    // Round 3 re-measurement (tools/ab_gemm_classes.py, M = 99 840, K = 512, class 1): since the 256^2 kernel's stores became
    // non-temporal it is the faster one here too -- 843 / 850 TF against gemm3's 775 / 798 (N = 2048 / 1536) -- so the default
    // rule is OFF; gemm3 stays reachable through I2T_GEMM3 for the record of the overlap experiment.
    const int cls = g256_epilogue_class(c);
    if (knobs.gemm3 && splits == 1 && !c.a_kmajor && !c.b_kmajor && c.K % 64 == 0 && c.alpha_one && !c.alpha_sumsq && (c.N & 7) == 0 &&
        (c.ldc & 7) == 0 && c.c_aligned16 &&
        ((cls == 1 && c.K >= 5 * 64) || (cls == 2 && c.K >= 8 * 64 && (!c.aux_out || ((c.ld_aux_out & 7) == 0 && c.aux_out_aligned16)))) &&
        (long)((c.M + 255) / 256) * ((c.N + 127) / 128) >= 2 * knobs.min_tiles) {
        r.kind = RouteKind::Gemm3;
        r.cls = cls;
        r.overlap = knobs.gemm3 == 2;
        return r;
    }
    // large-tile kernel for the non-split problems with enough 256^2 tiles to occupy the chip (I2T_GEMM=v1 keeps the 128^2 one)
    // K % 128 == 0 (K-tiles run in pairs and the DMA stream chains output tiles), or any K when B is k-major: the range check then
    // returns B rows >= K as zeros, so whatever finite values a row-major A delivers past K (its zero pads, then the head of the
    // next row) contribute nothing; k-major panels must fit a 32-bit byte offset
    const bool g256_ok = (c.K % 128 == 0 || c.b_kmajor) && (!c.a_kmajor || (unsigned long long)(c.K + 512) * c.lda * 2 < (1ull << 32)) &&
                         (!c.b_kmajor || (unsigned long long)(c.K + 512) * c.ldb * 2 < (1ull << 32));
    // N <= 128 (the LoRA adapters' rank-padded products u = x A^T, du = dY (s B)): a 256-column tile is half empty and M / 256 row tiles
    // leave most CUs idle -- the 128^2 kernel runs twice the workgroups on full tiles (I2T_G256_NARROW=1: the old routing, for A/B)
    if (splits == 1 && !knobs.no_g256 && g256_ok && !c.a_kmajor && (c.N > 128 || knobs.narrow_256) &&
        (long)((c.M + 255) / 256) * ((c.N + 255) / 256) >= knobs.min_tiles) {
        r.kind = RouteKind::G256;
        // forward GEMMs (B^T form) meet classes 1, 2, 3, 5, 7, the dX GEMMs (B form) classes 1, 4, 5; a class that is not built for
        // the layout runs the generic kernel (a wrong class would dereference a null epilogue operand)
        r.cls = (c.b_kmajor ? (cls == 2 || cls == 3 || cls == 7 || cls == 10) : (cls == 4 || cls == 11)) ? 0 : cls;
        return r;
    }
    r.kind = RouteKind::G128;
    r.splits = splits;
    return r;
}

}  // namespace i2t
