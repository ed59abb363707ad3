// Which kernels an i2t_attention_fwd / i2t_attention_bwd_ex / i2t_gq_attention_fwd / i2t_gq_attention_bwd call reaches: the whole
// decision, as plain C++17 on plain values (no HIP, no pointer is read), so that it runs on a CPU -- tests/test_attention_route_cpu.py
// holds a table of calls and the routes they must take.  attention.hip and attention_g.hip validate the arguments (attn_check),
// describe the call as an AttnCall, read the environment into AttnKnobs (attn_knobs, once per call), ask the route and launch what it says.
//
// The rule of the 64-wide heads, top to bottom (the first that applies).  "Resident" = the operands of one (sequence, head) fit the
// resident-operand kernels: I2T_ATTN_V2 is not 0, the call is dense (no cu_q / cu_k) and not causal, 64 <= Tq <= V2_MAX_OTHER (304),
// Tk <= V2_MAXROWS (288), and with dropout Tk % 4 == 0 (the 4 consecutive keys of a lane must be the 4 bytes of one hash).
//   forward   1. resident                          attn_fwd2_kernel<DROP, PER>, PER = ((Tq + 15) / 16) / 4 = 1 .. 4, one workgroup per (b, h);
//             2. everything else                   attn_fwd_kernel<DROP, EVEN>, one workgroup per 64 query rows.
//   backward  mode = I2T_ATTN_BWD (3 when unset), or 0 when I2T_ATTN_BWD2 is 0
//             1. mode 3, resident, Tq <= 288       attn_bwd3_kernel<DROP, NWV>, NWV = 9 only when I2T_ATTN_BWD3_WAVES asks for it, else 8;
//             2. mode != 0, resident, Tq <= 288    attn_bwd2_kernel<DROP>;
//             3. Tq <= 64, Tk <= 64                attn_bwd1_kernel<DROP, EVEN> unless I2T_ATTN_BWD1 is 0;
//             4. everything else                   attn_bwd_dq_kernel + attn_bwd_dkv_kernel<DROP, EVEN>.
//             out_drop_q_seq (0 when it equals Tq or there is no out-drop) is taken by route 1 alone: elsewhere the call is refused.
// <DROP, EVEN>: no dropout <false, true> | dropout and Tk % 4 == 0 <true, true> | dropout, any Tk <true, false>.
// The grouped-query path (any head width) has one kernel family: gattn_*_kernel<D, DROP>, D = 32 (hd <= 32), 64 or 128.
#pragma once

namespace i2t {

// Limits of the resident-operand kernels (the route and the kernels read the same numbers)
constexpr int V2_MAXROWS = 288, V2_RB = 128, V2_NQB = 4;              // rows staged in LDS, bytes per staged row, query blocks per wave
constexpr int V2_MAX_OTHER = 16 * (4 * V2_NQB + 3);                    // 304 rows of the per-wave operand

// One attention call, as far as routing reads it.  Pointers appear only as the facts taken from them.
struct AttnCall {
    int B, H, Hkv, hd;        // the 64-wide path: Hkv = H, hd = 64
    int Tq, Tk, causal;
    bool packed;              // cu_q or cu_k present
    bool drop;                // drop_thr != 0
    bool out_drop;            // out_drop_thr != 0 (backward)
    int out_drop_q_seq;       // as passed (i2t_attention_bwd_ex); attn_bwd_route normalises it
    int split;                // grouped-query forward: rows >= split do not see keys < split
};

// One field per I2T_* variable the attention host code reads (attention.hip::attn_knobs fills it, once per call).
struct AttnKnobs {
    bool v2;                  // I2T_ATTN_V2 does not start with '0': the resident-operand kernels may be used
    int bwd;                  // atoi(I2T_ATTN_BWD), 3 when unset: 3 the one-pass kernel | 2 (any other non-zero) the two-phase one | 0 the tiled ones
    bool bwd2;                // I2T_ATTN_BWD2 does not start with '0' (it does: as I2T_ATTN_BWD=0)
    bool bwd1;                // I2T_ATTN_BWD1 does not start with '0' (it does: the tiled pair on single-tile shapes, for A/B runs)
    int bwd3_waves;           // atoi(I2T_ATTN_BWD3_WAVES), 0 when unset: 9 asks for the 9-wave kernel, anything else runs 8
};

enum class AttnDrop { None, Even, Odd };      // the <DROP, EVEN> variant of a tiled kernel (EVEN only matters with dropout)

inline AttnDrop attn_drop_variant(const AttnCall& c) { return !c.drop ? AttnDrop::None : (c.Tk & 3) == 0 ? AttnDrop::Even : AttnDrop::Odd; }

// the resident-operand kernels cover dense, non-causal calls whose operands fit (the encoders); I2T_ATTN_V2=0 keeps the tiled ones
inline bool attn_resident(const AttnCall& c, const AttnKnobs& k) {
    return k.v2 && !c.causal && !c.packed && c.Tk <= V2_MAXROWS && c.Tq >= 64 && c.Tq <= V2_MAX_OTHER && (!c.drop || (c.Tk & 3) == 0);
}

enum class AttnFwdKind { Fwd2, Fwd };

struct AttnFwdRoute {
    AttnFwdKind kind;
    int per;                  // Fwd2: PER, sixteen-query blocks a wave owns (1 .. 4)
    AttnDrop drop;            // Fwd2 reads only dropout on / off (never Odd: a resident call with dropout has Tk % 4 == 0)
    int grid, block;
};

inline AttnFwdRoute attn_fwd_route(const AttnCall& c, const AttnKnobs& k) {
    if (attn_resident(c, k)) return {AttnFwdKind::Fwd2, ((c.Tq + 15) >> 4) >> 2, attn_drop_variant(c), c.H * c.B, 256};
    return {AttnFwdKind::Fwd, 0, attn_drop_variant(c), ((c.Tq + 63) / 64) * c.H * c.B, 256};
}

enum class AttnBwdKind { Bwd3, Bwd2, Bwd1, Pair };

struct AttnBwdRoute {
    AttnBwdKind kind;
    int nwv;                  // Bwd3: waves per workgroup (8 | 9)
    AttnDrop drop;            // Bwd3, Bwd2 read only dropout on / off
    int grid, grid_dkv;       // Pair: the dQ and the dK/dV launch; the others: grid alone
    int block;
    int q_seq;                // out_drop_q_seq as the kernel gets it: 0 when it equals Tq or there is no out-drop
    bool q_seq_ok;            // false: q_seq != 0 on a kernel that does not offer it -- the call is refused
};

inline AttnBwdRoute attn_bwd_route(const AttnCall& c, const AttnKnobs& k) {
    AttnBwdRoute r{};
    r.q_seq = (c.out_drop_q_seq == c.Tq || !c.out_drop) ? 0 : c.out_drop_q_seq;
    r.drop = attn_drop_variant(c);
    r.grid = r.grid_dkv = c.H * c.B;
    const int mode = k.bwd2 ? k.bwd : 0;
    const bool resident = attn_resident(c, k) && c.Tq <= V2_MAXROWS;
    if (mode == 3 && resident) {
        // 9 waves whenever 8 would leave a wave with a third key block (I2T_ATTN_BWD3_WAVES = 8 | 9 forces one: A/B runs)
        // measured (B = 1024, T = 260, dropout): 1295 us against 1228 for 8 waves -- the third register-limited
        // wave of a SIMD and its spills cost more than wave 0's third block: off unless asked for
        r.kind = AttnBwdKind::Bwd3;
        r.nwv = k.bwd3_waves == 9 ? 9 : 8;
        r.block = 64 * r.nwv;
        r.q_seq_ok = true;
        return r;
    }
    r.q_seq_ok = r.q_seq == 0;
    if (mode != 0 && resident) {
        r.kind = AttnBwdKind::Bwd2;
        r.block = 512;
        return r;
    }
    r.block = 256;
    // one tile of queries and keys (the decoder's attentions): the fused single-pass kernel (I2T_ATTN_BWD1=0: the tiled pair, for A/B runs)
    if (c.Tq <= 64 && c.Tk <= 64 && k.bwd1) {
        r.kind = AttnBwdKind::Bwd1;
        return r;
    }
    r.kind = AttnBwdKind::Pair;
    r.grid = ((c.Tq + 63) / 64) * c.H * c.B;
    r.grid_dkv = ((c.Tk + 63) / 64) * c.H * c.B;
    return r;
}

struct GqRoute {
    int d;                    // LDS tile width of the instantiation: 32 (a 16-wide head is a 32-wide one, upper half zero), 64 or 128
    bool drop;
    int grid_q;               // the forward and the dQ launch: one workgroup per 64 query rows of a query head
    int grid_dkv;             // one workgroup per 64 key rows of a key/value head
    int block;
};

inline GqRoute gq_route(const AttnCall& c) {
    return {c.hd <= 32 ? 32 : c.hd == 64 ? 64 : 128, c.drop, ((c.Tq + 63) / 64) * c.H * c.B, ((c.Tk + 63) / 64) * c.Hkv * c.B, 256};
}

}  // namespace i2t
