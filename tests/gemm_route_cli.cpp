// Stand-alone front end of image2text_amd/csrc/gemm_route.h for tests/test_gemm_route_cpu.py: no HIP, no GPU.
// stdin: one call per line, "name key=value ...".  stdout: "name route" per line.  Keys that are left out take the defaults below.
#include "../image2text_amd/csrc/gemm_route.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

using namespace i2t;

static const char* colsum_name(Colsum c) { return c == Colsum::None ? "none" : c == Colsum::Folded ? "folded" : "before"; }

static std::string plan_text(const DwPlan& p) {
    char b[96];
    snprintf(b, sizeof b, "%d/%d/%d/%s", p.cls, p.splits, p.per, colsum_name(p.colsum));
    return b;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string name, kv;
        if (!(in >> name) || name[0] == '#') continue;
        std::map<std::string, long> v;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: bad field %s\n", name.c_str(), kv.c_str()); return 2; }
            v[kv.substr(0, eq)] = atol(kv.c_str() + eq + 1);
        }
        auto get = [&](const char* key, long dflt) { auto it = v.find(key); if (it == v.end()) return dflt; long x = it->second; v.erase(it); return x; };
        auto r8 = [](long x) { return (x + 7) & ~7L; };
        GemmCall c{};
        c.M = (int)get("M", 1); c.N = (int)get("N", 1); c.K = (int)get("K", 1);
        c.a_kmajor = get("ak", 0) != 0; c.b_kmajor = get("bk", 0) != 0;
        c.lda = (int)get("lda", r8(c.a_kmajor ? c.M : c.K)); c.ldb = (int)get("ldb", r8(c.b_kmajor ? c.N : c.K)); c.ldc = (int)get("ldc", c.N);
        c.c_is_f32 = (int)get("f32", 0); c.accumulate = (int)get("acc", 0); c.act = (int)get("act", 0); c.drop_mode = (int)get("drop", 0);
        c.bias = get("bias", 0) != 0; c.aux_in = get("auxi", 0) != 0; c.aux_out = get("auxo", 0) != 0; c.residual = get("res", 0) != 0;
        c.ld_aux_in = (int)get("ldai", c.ldc); c.ld_aux_out = (int)get("ldao", c.ldc); c.ldr = (int)get("ldr", c.ldc);
        c.alpha_one = get("alpha1", 1) != 0; c.alpha_sumsq = get("as", 0) != 0; c.colsum_out = get("cso", 0) != 0;
        c.c_aligned16 = get("c16", 1) != 0; c.aux_out_aligned16 = get("auxo16", 1) != 0; c.residual_is_c = get("resc", 0) != 0;
        GemmKnobs k{};
        k.no_g256 = get("no_g256", 0) != 0; k.min_tiles = get("min_tiles", 40); k.gemm3 = (int)get("gemm3", 0); k.narrow_256 = get("narrow", 0) != 0;
        k.skinny_ksplit = get("ksplit", 0) != 0; k.fold_colsum = get("fold", 1) != 0; k.dw_splits = (int)get("dw_splits", 0);
        k.gn = (int)get("gn", 8); k.stagger = (int)get("stagger", 0); k.stagger_groups = (int)get("stagger_groups", 2); k.g256_dbg = (int)get("g256_dbg", 0);
        k.g3_dbg = (int)get("g3_dbg", 0); k.fp8_g256 = get("fp8_g256", 1) != 0; k.log = get("log", 0) != 0;
        const int n_cu = (int)get("n_cu", 256);
        const bool det = get("det", 0) != 0;
        if (!v.empty()) { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), v.begin()->first.c_str()); return 2; }

        const GemmRoute r = gemm_route(c, k, n_cu, det);
        printf("%s ", name.c_str());
        switch (r.kind) {
        case RouteKind::Skinny: printf("skinny mt=%d ksplit=%d", r.mt, r.ksplit); break;
        case RouteKind::DW:
            printf("dw kc=%ld chunks=%d full=%s", r.kc, r.chunks, plan_text(r.full).c_str());
            if (c.K % r.kc) printf(" tail=%s", plan_text(r.tail).c_str());
            if (r.chunk_error) printf(" error");
            break;
        case RouteKind::Gemm3: printf("gemm3 cls=%d overlap=%d", r.cls, (int)r.overlap); break;
        case RouteKind::G256: printf("g256 cls=%d", r.cls); break;
        case RouteKind::G128: printf("g128 splits=%d", r.splits); break;
        }
        if (r.kind != RouteKind::DW) printf(" colsum=%s", colsum_name(r.colsum));
        printf("\n");
    }
    return 0;
}
