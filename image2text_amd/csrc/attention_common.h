// Pieces shared by the head_dim-64 attention kernels (attention.hip) and the grouped-query / any-head-dim ones (attention_g.hip).
#pragma once
#include "common.h"
#include "attention_route.h"
#include <initializer_list>
#include <type_traits>

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct AttnPtr {
    const bf16_t* p;
    long bs;   // batch stride (elements)
    int rs;    // row stride (elements)
};

// Packed variable-length batches: sequence b owns rows [cu[b], cu[b+1]) of a [total, width] tensor (batch stride unused).
// cu_q / cu_k may be given independently (cross-attention: packed queries against fixed-length memories).
// With cu_q the per-row statistics (lse, delta) are laid out [H][total_q].
struct VarLen {
    const int* cu_q;
    const int* cu_k;
    int total_q;
    int nseq;                 // B: sequences in the batch (the 1-D grid decode needs it)
};

__device__ __forceinline__ bf16x8 pack_frag(const f32x4& a, const f32x4& b) {
    u32x4 v = {pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
    return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ float quad_max(float v) {   // across the 4 lanes that share a query column
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// Workgroup -> (tile, head, sequence) for a 1-D grid of ntile * H * B workgroups.  The tiles of one (head, sequence) pair
// re-read that pair's K and V (forward, dQ) or Q and dO (dK/dV) -- 5 times at T = 260.  Workgroups are dealt round-robin
// over the 8 XCDs by their linear id, so with the tile index fastest those 5 land on 5 different L2s and every re-read
// crosses the fabric (PMC: 6.3 GB per encoder layer forward against 2.2 GB algorithmic at B = 2048).  Here ids l, l + 8,
// l + 16, ... walk the tiles of ONE pair, i.e. one XCD serves all tiles of a pair back to back and its L2 absorbs the
// re-reads: FETCH_SIZE of the three kernels fell from 1840 to 906 MB per launch.  Their time did not move (VALU-bound, see
// below) -- kept for the fabric / HBM headroom it leaves to whatever runs beside them (the gradient exchange).  Placement
// affects speed only: any mapping gives the same result.
__device__ __forceinline__ void attn_block_coords(int ntile, int H, int B, int& tile, int& h, int& b) {
    const int L = blockIdx.x, P = H * B, full = (P >> 3) * 8 * ntile;
    int pair;
    if (L < full) {
        const int grp = L / (8 * ntile), r = L - grp * 8 * ntile;
        pair = grp * 8 + (r & 7);
        tile = r >> 3;
    } else {
        const int r = L - full;
        pair = (P >> 3) * 8 + r / ntile;
        tile = r % ntile;
    }
    h = pair % H;
    b = pair / H;
}

// ------------------------------------------------------------------------------------------------------------------ host side
// Each entry point validates (attn_check), describes the call (i2t::AttnCall), asks attention_route.h and launches what it says.

struct AttnOperand {
    const void* p;
    long bs;
    int rs, min_rs;           // min_rs: the columns a row must cover (64-wide path: 64; grouped path: heads x head width)
};

// The argument checks of the four entry points, stated once.  grouped: the any-head-width path (it also checks the head counts and
// the head width, and its rows must cover every head); backward: lse and the delta workspace (`stats`) are required.  The forward
// of the 64-wide path launches query tiles only, every other call also key tiles: hence the two grid sizes.
inline int attn_check(const char* who, const i2t::AttnCall& c, bool grouped, bool backward, const int* cu_q, int total_q, bool stats,
                      std::initializer_list<AttnOperand> operands) {
    I2T_REQUIRE(c.split == 0 || (!c.causal && !c.packed && c.Tq == c.Tk && c.split < c.Tq), "%s: split needs dense non-causal self-attention", who);
    const bool some = c.B > 0 && c.H > 0 && c.Hkv > 0 && c.Tq > 0 && c.Tk > 0;
    if (backward && !grouped) I2T_REQUIRE(some && stats, "%s: bad args", who);
    else I2T_REQUIRE(some, "%s: empty problem", who);
    if (grouped) {
        I2T_REQUIRE(c.H % c.Hkv == 0, "%s: H = %d is not a multiple of H_kv = %d", who, c.H, c.Hkv);
        I2T_REQUIRE(c.hd == 16 || c.hd == 32 || c.hd == 64 || c.hd == 128, "%s: head_dim %d (16, 32, 64 or 128)", who, c.hd);
    }
    I2T_REQUIRE(!cu_q || total_q > 0, "%s: packed queries need total_q", who);
    I2T_REQUIRE(!c.drop || (double)c.B * c.H * c.Tq * c.Tk < 4294967296.0, "%s: dropout index overflows 32 bits", who);
    I2T_REQUIRE(!c.causal || c.Tk >= c.Tq, "%s: causal needs Tk >= Tq", who);
    const int tiles = (c.Tq + 63) / 64 + (grouped || backward ? (c.Tk + 63) / 64 : 0);
    I2T_REQUIRE((double)tiles * c.H * c.B < 2147483647.0, "%s: grid too large", who);
    if (grouped && backward) I2T_REQUIRE(stats, "%s: lse and the delta workspace are required", who);
    bool ok = true;
    for (const AttnOperand& o : operands) ok = ok && o.p && ALIGNED16(o.p) && (o.bs % 8 == 0) && (o.rs % 8 == 0) && o.rs >= o.min_rs;
    I2T_REQUIRE(ok, grouped ? "%s: operands must be 16-byte aligned with strides that are multiples of 8 and cover every head"
                            : "%s: operands must be 16-byte aligned with strides that are multiples of 8", who);
    return I2T_OK;
}

// A runtime value as a template argument: calls f(std::integral_constant<T, V>{}) for the V of the list that equals v (none: no call).
// A kernel template is launched inside a generic lambda, with decltype(arg)::value as its template arguments.
template <auto... Vs, class T, class F>
inline void with_constant(T v, F&& f) {
    (void)((v == Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}

// f(DROP, EVEN) for the <bool DROP, bool EVEN> variant of a tiled 64-wide kernel (EVEN = Tk % 4 == 0; only matters with dropout)
template <class F>
inline void with_drop_variant(i2t::AttnDrop d, F&& f) {
    with_constant<i2t::AttnDrop::None, i2t::AttnDrop::Even, i2t::AttnDrop::Odd>(d, [&](auto V) {
        f(std::bool_constant<decltype(V)::value != i2t::AttnDrop::None>{}, std::bool_constant<decltype(V)::value != i2t::AttnDrop::Odd>{});
    });
}

}  // namespace
