// Stand-alone front end of image2text_amd/csrc/conv_route.h for tests/test_conv_route_cpu.py: no HIP, no GPU.
// stdin: one call per line, "name op=fwd|bwd_data|bwd_weight|transpose|gfwd|gbwd_data|gbwd_weight key=value ..." (g...: the generic path of
// conv.hip).  stdout: "name route" per line: every launch the entry point makes, in order, as kernel<template arguments> grid block and
// the integer arguments it is handed, "memset bytes=N" for the scratch memset; or "refused: text".  Keys that are left out take the
// defaults below.  With the argument --set: the instantiated set instead, one kernel per line with the workspace it needs.
#include "../image2text_amd/csrc/conv_route.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

using namespace i2t;

static const char* tf(bool b) { return b ? "true" : "false"; }

static std::string fmt(const char* f, ...) {
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

static std::string launch(const std::string& kernel, ConvGrid g, int block, const std::string& args) {
    return kernel + fmt(" grid=(%d,%d,%d) block=%d args=(", g.x, g.y, g.z, block) + args + ")";
}

static std::string name6(const Conv6Targs& t, bool spelled) {
    static const char* src[] = {"SRC_NCHW_F32", "SRC_NCHW_BF16", "SRC_NHWC_BF16"};
    if (spelled) return fmt("conv_mfma_kernel<%d, %d, %s, %s, %s, %s>", t.CP, t.NT, src[t.SRC], tf(t.IN_GELU), tf(t.DGELU), tf(t.DST_NCHW));
    return fmt("conv_mfma_kernel<%d,%d,%d,%s,%s,%s,%d,%d>", t.CP, t.NT, t.SRC, tf(t.IN_GELU), tf(t.DGELU), tf(t.DST_NCHW), t.NW, t.GRP);
}

static std::string name6bw(const Conv6BwdWeightTargs& t, bool spelled) {
    static const char* src[] = {"SRC_NCHW_F32", "SRC_NCHW_BF16", "SRC_NHWC_BF16"};
    if (spelled) return fmt("conv_mfma_bwd_weight_kernel<%d, %d, %s, %s, %s>", t.CP, t.COP, src[t.DY_SRC], src[t.ACT_SRC], tf(t.ACT_GELU));
    return fmt("conv_mfma_bwd_weight_kernel<%d,%d,%d,%d,%s>", t.CP, t.COP, t.DY_SRC, t.ACT_SRC, tf(t.ACT_GELU));
}

static std::string conv6_text(const ConvCall& c) {
    const Conv6Route r = conv6_route(c);
    if (r.refused[0]) return std::string("refused: ") + r.refused;
    return launch("conv_repack_kernel", {64, 1, 1}, 256, fmt("%d,%d,%d,%d,%d", c.Cout, c.Cin, r.rows_p, r.red_p, r.flip)) + " + " +
           launch(name6(r.t, false), r.grid, r.block, fmt("%d,%d,%d,%d,%d,%d", r.cin, r.cout, c.H, c.W, r.pad_before, r.tiles_x));
}

static std::string conv6_bwd_weight_text(const ConvCall& c, bool det) {
    const Conv6BwdWeightRoute r = conv6_bwd_weight_route(c, det);
    if (r.refused[0]) return std::string("refused: ") + r.refused;
    std::string out = fmt("memset bytes=%zu", r.scratch_bytes);
    for (int bz = 0; bz < r.serial.y; ++bz)
        for (int by = 0; by < r.serial.x; ++by)
            out += " + " + launch(name6bw(r.t, false), r.grid, r.block, fmt("%d,%d,%d,%d,%d,%d,%d,%d", c.Cin, c.Cout, c.H, c.W, r.pad_before, r.tiles_x, by, bz));
    return out + " + " + launch("conv_fold_dw_kernel", {32, 1, 1}, 256, fmt("%d,%d,%d", c.Cout, c.Cin, r.t.CP));
}

static std::string transpose_text(const ConvCall& c) {
    const TransposeRoute r = nchw_to_nhwc_route(c);
    if (r.refused[0]) return std::string("refused: ") + r.refused;
    return r.c32 ? launch("nchw_to_nhwc32_kernel", r.grid, r.block, fmt("%d,%d", c.H, c.W))
                 : launch("nchw_to_nhwc_kernel", r.grid, r.block, fmt("%d,%d,%d", c.Cin, c.H, c.W));
}

static std::string direct_text(const ConvCall& c) {
    const ConvDirectRoute r = conv_direct_route(c);
    if (r.refused[0]) return std::string("refused: ") + r.refused;
    return launch("repack_weights_kernel", {32, 1, 1}, 256, fmt("%d,%d,%d,%d", c.Cout, c.Cin, c.k, r.flip)) + " + " +
           launch(fmt("conv_direct_kernel<%d,%d,%s,%s,%s>", r.t.COUT_T, r.t.K, tf(r.t.IN_F32), tf(r.t.IN_GELU), tf(r.t.DGELU)), r.grid, r.block,
                  fmt("%d,%d,%d,%d,%d,%d", r.cin, r.cout, c.H, c.W, r.pad_before, r.groups));
}

static std::string direct_bwd_weight_text(const ConvCall& c, bool det) {
    const ConvDirectBwdWeightRoute r = conv_direct_bwd_weight_route(c, det);
    if (r.refused[0]) return std::string("refused: ") + r.refused;
    std::string out;
    for (int bz = 0; bz < r.serial.z; ++bz)
        for (int by = 0; by < r.serial.y; ++by)
            for (int bx = 0; bx < r.serial.x; ++bx)
                out += (out.empty() ? "" : " + ") + launch(fmt("conv_bwd_weight_kernel<%d,%d,%s,%s>", r.t.COUT, r.t.K, tf(r.t.IN_F32), tf(r.t.IN_GELU)), r.grid, r.block,
                                                           fmt("%d,%d,%d,%d,%d,%d,%d", c.Cin, c.H, c.W, r.pad_before, bx, by, bz));
    return out;
}

// the instantiated set, by walking the candidates the launchers walk under the predicates they use
static void print_set() {
    for (int i = 0; i < CONV6_CANDIDATES; ++i) {
        const Conv6Targs t = conv6_candidate(i);
        if (conv6_instantiated(t)) printf("%s NW=%d GRP=%d ws_elems=%d\n", name6(t, true).c_str(), t.NW, t.GRP, 16 * t.NT * NTAP * t.CP);
    }
    for (int i = 0; i < CONV6_BWD_WEIGHT_CANDIDATES; ++i) {
        const Conv6BwdWeightTargs t = conv6_bwd_weight_candidate(i);
        if (conv6_bwd_weight_instantiated(t)) printf("%s scratch_floats=%d\n", name6bw(t, true).c_str(), t.COP * NTAP * t.CP);
    }
    printf("nchw_to_nhwc32_kernel\nnchw_to_nhwc_kernel\n");
    for (int i = 0; i < CONV_DIRECT_CANDIDATES; ++i) {
        const ConvDirectTargs t = conv_direct_candidate(i);
        if (conv_direct_instantiated(t)) printf("conv_direct_kernel<%d, %d, %s, %s, %s>\n", t.COUT_T, t.K, tf(t.IN_F32), tf(t.IN_GELU), tf(t.DGELU));
    }
    for (int i = 0; i < CONV_DIRECT_BWD_WEIGHT_CANDIDATES; ++i) {
        const ConvDirectBwdWeightTargs t = conv_direct_bwd_weight_candidate(i);
        if (conv_direct_bwd_weight_instantiated(t)) printf("conv_bwd_weight_kernel<%d, %d, %s, %s>\n", t.COUT, t.K, tf(t.IN_F32), tf(t.IN_GELU));
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--set")) {
        print_set();
        return 0;
    }
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string name, kv;
        if (!(in >> name) || name[0] == '#') continue;
        std::map<std::string, std::string> v;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: bad field %s\n", name.c_str(), kv.c_str()); return 2; }
            v[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        auto get = [&](const char* key, long dflt) { auto it = v.find(key); if (it == v.end()) return dflt; long x = atol(it->second.c_str()); v.erase(it); return x; };
        std::string op = "fwd";
        if (v.count("op")) { op = v["op"]; v.erase("op"); }
        const bool generic = op[0] == 'g';
        const std::string what = generic ? op.substr(1) : op;
        ConvCall c{};
        c.op = what == "bwd_data" ? ConvOp::BwdData : what == "bwd_weight" ? ConvOp::BwdWeight : ConvOp::Fwd;
        // xl, dyl: the layouts as the MFMA entry points take them; the generic entry points take f32 (in_is_f32) instead, their dY is NCHW bf16
        c.x_layout = generic ? (get("f32", 0) ? SRC_NCHW_F32 : SRC_NCHW_BF16) : (int)get("xl", SRC_NHWC_BF16);
        c.dy_layout = generic ? SRC_NCHW_BF16 : (int)get("dyl", SRC_NHWC_BF16);
        c.in_gelu = get("gelu", 0) != 0; c.pre = get("pre", 1) != 0; c.dst_nchw = get("nchw", 0) != 0;
        c.B = (int)get("B", 1); c.Cin = (int)get("Cin", 8); c.Cout = (int)get("Cout", 16); c.H = (int)get("H", 16); c.W = (int)get("W", 16);
        c.k = (int)get("k", KS); c.aligned16 = get("aligned", 1) != 0;
        const bool det = get("det", 0) != 0, pointers = get("ptr", 1) != 0;
        if (op == "transpose") c.Cin = c.Cout = (int)get("C", 32);
        if (!v.empty()) { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), v.begin()->first.c_str()); return 2; }
        std::string route;
        const ConvChecked chk = conv_check(c, pointers);
        if (chk.refused[0]) route = std::string("refused: ") + chk.refused;
        else if (op == "fwd" || op == "bwd_data") route = conv6_text(c);
        else if (op == "bwd_weight") route = conv6_bwd_weight_text(c, det);
        else if (op == "transpose") route = transpose_text(c);
        else if (op == "gfwd" || op == "gbwd_data") route = direct_text(c);
        else if (op == "gbwd_weight") route = direct_bwd_weight_text(c, det);
        else { fprintf(stderr, "%s: unknown op %s\n", name.c_str(), op.c_str()); return 2; }
        printf("%s %s\n", name.c_str(), route.c_str());
    }
    return 0;
}
