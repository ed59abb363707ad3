// Which kernels an i2t_conv6_fwd / i2t_conv6_bwd_data / i2t_conv6_bwd_weight / i2t_nchw_to_nhwc_bf16 call (conv_mfma.hip) and an
// i2t_conv_fwd / i2t_conv_bwd_data / i2t_conv_bwd_weight call (conv.hip, the generic path) reaches: the whole decision, as plain C++17
// on plain values (no HIP, no pointer is read), so that it runs on a CPU -- tests/test_conv_route_cpu.py holds a table of calls and the
// launches they must make.  Each entry point describes its call as a ConvCall, runs conv_check (pointers present, every size positive),
// asks the route and launches what it says; a call that is refused -- by the check or by the route -- has issued nothing.
//
// The 6x6 MFMA kernels.  CP = pad8(reduction channels) = 8 | 16 | 32, output channels padded to 16 NT (NT = 1 up to 16, else 2).
//   forward        Cin, Cout <= 32.  An NHWC source has exactly 8 / 16 / 32 channels, an NHWC output Cout % 8 == 0.  Then
//                  the fp32 NCHW image, no GELU, CP = 8       conv_mfma_kernel<8, NT, SRC_NCHW_F32, false, false, DST_NCHW>
//                  an NHWC bf16 pre-activation through GELU   conv_mfma_kernel<CP, NT, SRC_NHWC_BF16, true, false, DST_NCHW>
//                  anything else is refused (unsupported layout combination).  Padding 2 before.
//   backward-data  the forward with the roles swapped: the kernel's source is dY (NCHW bf16, or NHWC bf16 with exactly 8 / 16 / 32
//                  channels), its reduction runs over the forward's Cout (<= 32), its output channels are the forward's Cin (8 or 16:
//                  NT = 1), the weights are repacked mirrored (flip), the padding is mirrored (3 before), and the epilogue multiplies
//                  by GELU' of the stored pre-activation into an NHWC dX:   conv_mfma_kernel<CP, 1, DY layout, false, true, false>
//   both           NW = 8 waves (512 threads) for CP = 32 and for an NCHW output at CP = 16, else 4 (256); the NCHW store group GRP is
//                  CONV_NCHW_GRP for an NCHW output at CP >= 16, else 1; one workgroup per (tile row, image); the weights are
//                  repacked to rows_p x 36 x red_p bf16 in the caller's workspace first.
//   backward-weight  Cin <= 16, Cout <= 32, COP = 16 | 32; an NHWC dY has Cout % 8 == 0 (any other dY layout is read as NCHW bf16).
//                  the fp32 NCHW image, no GELU, CP = 8       conv_mfma_bwd_weight_kernel<8, COP, DY, SRC_NCHW_F32, false>
//                  an NHWC activation through GELU, Cin 8|16  conv_mfma_bwd_weight_kernel<CP, COP, DY, SRC_NHWC_BF16, true>
//                  memset of the COP x 36 x CP fp32 scratch, the kernel over (tile row, image), conv_fold_dw_kernel.  Deterministic
//                  mode: one single-workgroup launch per (image, tile row), images outermost, so the atomics land in a fixed order.
//   transpose      C <= 32.  C == 32, W % 8 == 0, both pointers 16-byte aligned: nchw_to_nhwc32_kernel; else nchw_to_nhwc_kernel.
// The generic path (k = 4 | 6, NCHW tensors, 32 x 32 tiles): conv_direct_kernel<COUT_T, K, IN_F32, IN_GELU, DGELU>, COUT_T = 4 | 8 | 16
// output channels per workgroup (the smallest that holds Cout, 16 beyond), backward-data again as the forward with the roles swapped
// and, when the layer's input went through GELU, DGELU on the stored pre-activation; conv_bwd_weight_kernel<COUT, K, IN_F32, IN_GELU>
// for Cout = 4 | 8 | 16 | 32 and every input form but fp32 + GELU, serial over (image, tile row, tile column) in deterministic mode.
//
// Which tuples of template arguments the library instantiates is stated once, by the *_instantiated predicates: the routes return only
// members, and the launchers walk the *_candidate lists under `if constexpr (..._instantiated(..))`, so no other kernel is compiled.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <utility>

#ifndef CONV_NCHW_GRP           // tools/build_variant.sh: -DCONV_NCHW_GRP=... builds an A/B variant
#define CONV_NCHW_GRP 4
#endif

namespace i2t {

// ---- the numbers the kernels and the routes share
constexpr int TS = 16;            // conv_mfma.hip: output tile edge
constexpr int KS = 6;             // conv_mfma.hip: kernel size
constexpr int NTAP = KS * KS;
constexpr int TILE = 32;          // conv.hip: output tile edge
constexpr int NCHW_GRP = CONV_NCHW_GRP;      // conv_mfma_kernel: tiles of an NCHW output held and stored together
enum { SRC_NCHW_F32 = 0, SRC_NCHW_BF16 = 1, SRC_NHWC_BF16 = 2 };      // include/i2t.h I2T_LAYOUT_*

constexpr int pad8(int c) { return c <= 8 ? 8 : (c <= 16 ? 16 : 32); }
constexpr int cop16(int c) { return c <= 16 ? 16 : 32; }                // output channels padded to MFMA tiles
constexpr int tiles(int n, int tile) { return (n + tile - 1) / tile; }

// One convolution call, as far as routing reads it.  Pointers appear only as the facts taken from them.
enum class ConvOp { Fwd, BwdData, BwdWeight };
struct ConvCall {
    ConvOp op;
    int x_layout;             // SRC_* of the layer's input (fwd, bwd_weight; the generic path: SRC_NCHW_F32 | SRC_NCHW_BF16)
    int dy_layout;            // SRC_* of dY (bwd_data, bwd_weight)
    bool in_gelu;             // the layer's input is a stored pre-activation: GELU while staging (generic bwd_data: GELU' on the way out)
    bool pre;                 // bwd_data: the stored pre-activation is present
    bool dst_nchw;            // fwd: the output is written NCHW
    int B, Cin, Cout, H, W;   // of the forward convolution; the transpose: C = Cin
    int k;                    // kernel size (the generic path; the MFMA path is KS)
    bool aligned16;           // the transpose: source and destination are 16-byte aligned
};

struct ConvGrid {
    int x, y, z;
};

// A refusal is its text (without the entry point's name, which the caller puts in front); an accepted call has none.
constexpr int CONV_WHY = 160;
template <class R>
inline R conv_refuse(const char* fmt, ...) {
    R r{};
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.refused, sizeof r.refused, fmt, ap);
    va_end(ap);
    return r;
}
template <class R>
inline R conv_bad_args() { return conv_refuse<R>("bad args"); }

struct ConvChecked {
    char refused[CONV_WHY];
};
// The argument check of all seven entry points: every pointer the call needs is there (`pointers`) and no size is empty.
inline ConvChecked conv_check(const ConvCall& c, bool pointers) {
    if (!(pointers && c.B > 0 && c.Cin > 0 && c.Cout > 0 && c.H > 0 && c.W > 0)) return conv_bad_args<ConvChecked>();
    return ConvChecked{};
}

// f(std::integral_constant<int, i>) for i = N - 1 .. 0 until one returns true: how a launcher turns a route's run-time template
// arguments into the instantiation (and the only place a kernel template is named with them).  Downwards, because hipcc emits the
// instantiations it meets in a fold last to first: the kernels then stand in the code object in candidate order.
template <class F, int... Is>
inline bool first_index_impl(F&& f, std::integer_sequence<int, Is...>) {
    return (f(std::integral_constant<int, (int)sizeof...(Is) - 1 - Is>{}) || ...);
}
template <int N, class F>
inline bool first_index(F&& f) { return first_index_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{}); }

// ------------------------------------------------------------------------------------------- conv_mfma_kernel (fwd / bwd-data)
struct Conv6Targs {
    int CP, NT, SRC;
    bool IN_GELU, DGELU, DST_NCHW;
    int NW, GRP;              // follow from CP and DST_NCHW (conv6_targs)
};
constexpr Conv6Targs conv6_targs(int CP, int NT, int SRC, bool G, bool D, bool N) {
    return {CP, NT, SRC, G, D, N, (CP == 32 || (N && CP == 16)) ? 8 : 4, (N && CP >= 16) ? NCHW_GRP : 1};
}
constexpr bool same(const Conv6Targs& a, const Conv6Targs& b) {
    return a.CP == b.CP && a.NT == b.NT && a.SRC == b.SRC && a.IN_GELU == b.IN_GELU && a.DGELU == b.DGELU && a.DST_NCHW == b.DST_NCHW;
}
// the image (CP = 8, no GELU) | an NHWC pre-activation through GELU | backward-data: a bf16 dY, GELU' epilogue, one 16-channel NHWC tile
constexpr bool conv6_instantiated(int CP, int NT, int SRC, bool G, bool D, bool N) {
    if (!(CP == 8 || CP == 16 || CP == 32) || !(NT == 1 || NT == 2)) return false;
    if (D) return NT == 1 && !G && !N && (SRC == SRC_NCHW_BF16 || SRC == SRC_NHWC_BF16);
    if (SRC == SRC_NCHW_F32) return CP == 8 && !G;
    return SRC == SRC_NHWC_BF16 && G;
}
constexpr bool conv6_instantiated(const Conv6Targs& t) { return conv6_instantiated(t.CP, t.NT, t.SRC, t.IN_GELU, t.DGELU, t.DST_NCHW); }
constexpr int CONV6_CANDIDATES = 2 * 3 * 2 * 2 * 3 * 2;
constexpr Conv6Targs conv6_candidate(int i) {             // DGELU, SRC, IN_GELU, DST_NCHW, CP, NT: the last runs fastest
    return conv6_targs(8 << ((i / 2) % 3), 1 + i % 2, (i / 24) % 3, (i / 12) % 2 != 0, i / 72 != 0, (i / 6) % 2 != 0);
}

struct Conv6Route {
    char refused[CONV_WHY];
    Conv6Targs t;
    int cin, cout;            // as the kernel gets them: bwd_data swaps the roles
    ConvGrid grid;
    int block, pad_before, tiles_x;
    int rows_p, red_p, flip;  // conv_repack_kernel: the workspace takes rows_p x NTAP x red_p bf16
    size_t ws_elems;
};

inline Conv6Route conv6_route(const ConvCall& c) {
    using R = Conv6Route;
    const bool fwd = c.op == ConvOp::Fwd;
    if (fwd) {
        if (c.Cin > 32 || c.Cout > 32) return conv_bad_args<R>();
        if (c.x_layout == SRC_NHWC_BF16 && c.Cin != pad8(c.Cin)) return conv_refuse<R>("NHWC input needs 8/16/32 channels");
        if (!c.dst_nchw && c.Cout % 8 != 0) return conv_refuse<R>("NHWC output needs Cout %% 8 == 0");
    } else {
        if (!c.pre || c.Cin % 8 != 0 || c.Cin > 16 || c.Cout > 32) return conv_bad_args<R>();
        if (!(c.dy_layout == SRC_NCHW_BF16 || (c.dy_layout == SRC_NHWC_BF16 && c.Cout == pad8(c.Cout)))) return conv_refuse<R>("dy layout");
    }
    R r{};
    // backward-data is the forward on dY with the roles swapped: reduction over Cout, Cin output channels, mirrored taps and padding
    r.cin = fwd ? c.Cin : c.Cout;
    r.cout = fwd ? c.Cout : c.Cin;
    const int src = fwd ? c.x_layout : c.dy_layout;
    const bool gelu = fwd && c.in_gelu, dgelu = !fwd, nchw = fwd && c.dst_nchw;
    r.t = conv6_targs(pad8(r.cin), r.cout <= 16 ? 1 : 2, src, gelu, dgelu, nchw);
    if (!conv6_instantiated(r.t))
        return conv_refuse<R>("unsupported layout combination (src=%d gelu=%d dgelu=%d nchw_out=%d)", src, (int)gelu, (int)dgelu, (int)nchw);
    r.pad_before = fwd ? (KS - 1) / 2 : KS - 1 - (KS - 1) / 2;
    r.tiles_x = tiles(c.W, TS);
    r.grid = {tiles(c.H, TS), c.B, 1};
    r.block = 64 * r.t.NW;
    r.rows_p = 16 * r.t.NT;
    r.red_p = r.t.CP;
    r.flip = fwd ? 0 : 1;
    r.ws_elems = (size_t)r.rows_p * NTAP * r.red_p;
    return r;
}

// ------------------------------------------------------------------------------------------------ conv_mfma_bwd_weight_kernel
struct Conv6BwdWeightTargs {
    int CP, COP, DY_SRC, ACT_SRC;
    bool ACT_GELU;
};
constexpr bool same(const Conv6BwdWeightTargs& a, const Conv6BwdWeightTargs& b) {
    return a.CP == b.CP && a.COP == b.COP && a.DY_SRC == b.DY_SRC && a.ACT_SRC == b.ACT_SRC && a.ACT_GELU == b.ACT_GELU;
}
constexpr bool conv6_bwd_weight_instantiated(int CP, int COP, int DY, int ACT, bool G) {
    if (!(CP == 8 || CP == 16) || !(COP == 16 || COP == 32) || !(DY == SRC_NCHW_BF16 || DY == SRC_NHWC_BF16)) return false;
    return ACT == SRC_NCHW_F32 ? (CP == 8 && !G) : (ACT == SRC_NHWC_BF16 && G);
}
constexpr bool conv6_bwd_weight_instantiated(const Conv6BwdWeightTargs& t) { return conv6_bwd_weight_instantiated(t.CP, t.COP, t.DY_SRC, t.ACT_SRC, t.ACT_GELU); }
constexpr int CONV6_BWD_WEIGHT_CANDIDATES = 3 * 2 * 2 * 3 * 2;
constexpr Conv6BwdWeightTargs conv6_bwd_weight_candidate(int i) {      // ACT_SRC, ACT_GELU, CP, DY_SRC (NHWC first), COP: the last runs fastest
    return {8 << ((i / 6) % 2), 16 << (i % 2), 2 - (i / 2) % 3, (i / 24) % 3, (i / 12) % 2 != 0};
}

struct Conv6BwdWeightRoute {
    char refused[CONV_WHY];
    Conv6BwdWeightTargs t;
    ConvGrid grid;            // of one launch
    ConvGrid serial;          // launches: for z, for y, for x (x fastest), the kernel's block offsets (by0 = x, bz0 = y); {1, 1, 1}: one launch
    int block, pad_before, tiles_x;
    size_t scratch_bytes;     // memset before the launches, folded into dW after them
};

inline Conv6BwdWeightRoute conv6_bwd_weight_route(const ConvCall& c, bool det) {
    using R = Conv6BwdWeightRoute;
    if (c.Cin > 16 || c.Cout > 32) return conv_bad_args<R>();
    if (c.dy_layout == SRC_NHWC_BF16 && c.Cout % 8 != 0) return conv_refuse<R>("NHWC dy needs Cout %% 8 == 0");
    R r{};
    r.t = {pad8(c.Cin), cop16(c.Cout), c.dy_layout == SRC_NHWC_BF16 ? SRC_NHWC_BF16 : SRC_NCHW_BF16, c.x_layout, c.in_gelu};
    if (!conv6_bwd_weight_instantiated(r.t) || (c.x_layout == SRC_NHWC_BF16 && c.Cin != r.t.CP))
        return conv_refuse<R>("unsupported layout combination (x_layout=%d gelu=%d Cin=%d)", c.x_layout, (int)c.in_gelu, c.Cin);
    const ConvGrid all = {tiles(c.H, TS), c.B, 1};
    r.grid = det ? ConvGrid{1, 1, 1} : all;
    r.serial = det ? all : ConvGrid{1, 1, 1};
    r.block = 256;
    r.pad_before = (KS - 1) / 2;
    r.tiles_x = tiles(c.W, TS);
    r.scratch_bytes = sizeof(float) * (size_t)r.t.COP * NTAP * r.t.CP;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- transpose
struct TransposeRoute {
    char refused[CONV_WHY];
    bool c32;                 // nchw_to_nhwc32_kernel (16-byte accesses both ways) | nchw_to_nhwc_kernel
    ConvGrid grid;
    int block;
};

inline TransposeRoute nchw_to_nhwc_route(const ConvCall& c) {
    if (c.Cin > 32) return conv_bad_args<TransposeRoute>();
    TransposeRoute r{};
    r.c32 = c.Cin == 32 && c.W % 8 == 0 && c.aligned16;
    r.grid = {tiles(c.W, 64), c.H, c.B};
    r.block = 256;
    return r;
}

// ------------------------------------------------------------------------------------- the generic path: conv_direct_kernel
struct ConvDirectTargs {
    int COUT_T, K;
    bool IN_F32, IN_GELU, DGELU;
};
constexpr bool same(const ConvDirectTargs& a, const ConvDirectTargs& b) {
    return a.COUT_T == b.COUT_T && a.K == b.K && a.IN_F32 == b.IN_F32 && a.IN_GELU == b.IN_GELU && a.DGELU == b.DGELU;
}
constexpr bool conv_direct_instantiated(int COUT_T, int K, bool F, bool G, bool D) {
    return (COUT_T == 4 || COUT_T == 8 || COUT_T == 16) && (K == 4 || K == 6) && (!D || (!F && !G));
}
constexpr bool conv_direct_instantiated(const ConvDirectTargs& t) { return conv_direct_instantiated(t.COUT_T, t.K, t.IN_F32, t.IN_GELU, t.DGELU); }
constexpr int CONV_DIRECT_CANDIDATES = 2 * 2 * 2 * 3 * 2;
constexpr ConvDirectTargs conv_direct_candidate(int i) {               // input form, COUT_T, K (6 first): the last runs fastest
    constexpr int form[8] = {4, 2, 0, 6, 1, 5, 3, 7};                  // IN_F32 = 4 | IN_GELU = 2 | DGELU = 1: the five members first
    return {4 << ((i / 2) % 3), 6 - 2 * (i % 2), (form[i / 6] & 4) != 0, (form[i / 6] & 2) != 0, (form[i / 6] & 1) != 0};
}

struct ConvDirectRoute {
    char refused[CONV_WHY];
    ConvDirectTargs t;
    int cin, cout;            // as the kernel gets them: bwd_data swaps the roles
    ConvGrid grid;
    int block, pad_before, groups;
    int flip;                 // repack_weights_kernel
};

inline ConvDirectRoute conv_direct_route(const ConvCall& c) {
    using R = ConvDirectRoute;
    const bool fwd = c.op == ConvOp::Fwd;
    if (!fwd && c.in_gelu && !c.pre) return conv_refuse<R>("in_gelu needs the stored pre-activation");
    if (c.k != 4 && c.k != 6) return conv_refuse<R>("kernel size %d unsupported (4 or 6)", c.k);
    R r{};
    r.cin = fwd ? c.Cin : c.Cout;
    r.cout = fwd ? c.Cout : c.Cin;
    r.t = {r.cout <= 4 ? 4 : (r.cout <= 8 ? 8 : 16), c.k, fwd && c.x_layout == SRC_NCHW_F32, fwd && c.in_gelu, !fwd && c.in_gelu};
    r.groups = tiles(r.cout, r.t.COUT_T);
    r.grid = {tiles(c.W, TILE), tiles(c.H, TILE), c.B * r.groups};
    r.block = 256;
    r.pad_before = fwd ? (c.k - 1) / 2 : c.k - 1 - (c.k - 1) / 2;      // backward-data: mirrored
    r.flip = fwd ? 0 : 1;
    return r;
}

// ----------------------------------------------------------------------------------- the generic path: conv_bwd_weight_kernel
struct ConvDirectBwdWeightTargs {
    int COUT, K;
    bool IN_F32, IN_GELU;
};
constexpr bool same(const ConvDirectBwdWeightTargs& a, const ConvDirectBwdWeightTargs& b) {
    return a.COUT == b.COUT && a.K == b.K && a.IN_F32 == b.IN_F32 && a.IN_GELU == b.IN_GELU;
}
constexpr bool conv_direct_bwd_weight_instantiated(int COUT, int K, bool F, bool G) {
    return (COUT == 4 || COUT == 8 || COUT == 16 || COUT == 32) && (K == 4 || K == 6) && !(F && G);
}
constexpr bool conv_direct_bwd_weight_instantiated(const ConvDirectBwdWeightTargs& t) { return conv_direct_bwd_weight_instantiated(t.COUT, t.K, t.IN_F32, t.IN_GELU); }
constexpr int CONV_DIRECT_BWD_WEIGHT_CANDIDATES = 2 * 4 * 2 * 2;
constexpr ConvDirectBwdWeightTargs conv_direct_bwd_weight_candidate(int i) {      // K (6 first), COUT, input form: the last runs fastest
    constexpr int form[4] = {2, 1, 0, 3};                              // IN_F32 = 2 | IN_GELU = 1: the three members first
    return {4 << ((i / 4) % 4), 6 - 2 * (i / 16), (form[i % 4] & 2) != 0, (form[i % 4] & 1) != 0};
}

struct ConvDirectBwdWeightRoute {
    char refused[CONV_WHY];
    ConvDirectBwdWeightTargs t;
    ConvGrid grid;            // of one launch
    ConvGrid serial;          // launches: for z, for y, for x (x fastest), the kernel's block offsets (bx0, by0, bz0); {1, 1, 1}: one launch
    int block, pad_before;
};

inline ConvDirectBwdWeightRoute conv_direct_bwd_weight_route(const ConvCall& c, bool det) {
    using R = ConvDirectBwdWeightRoute;
    const bool f32 = c.x_layout == SRC_NCHW_F32;
    if (f32 && c.in_gelu) return conv_refuse<R>("f32+gelu input combination unsupported");
    R r{};
    r.t = {c.Cout, c.k, f32, c.in_gelu};
    if (!conv_direct_bwd_weight_instantiated(r.t)) return conv_refuse<R>("Cout=%d k=%d unsupported (Cout in {4,8,16,32}, k in {4,6})", c.Cout, c.k);
    const ConvGrid all = {tiles(c.W, TILE), tiles(c.H, TILE), c.B};
    r.grid = det ? ConvGrid{1, 1, 1} : all;
    r.serial = det ? all : ConvGrid{1, 1, 1};
    r.block = 256;
    r.pad_before = (c.k - 1) / 2;
    return r;
}

}  // namespace i2t
