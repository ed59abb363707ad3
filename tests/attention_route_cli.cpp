// Stand-alone front end of image2text_amd/csrc/attention_route.h for tests/test_attention_route_cpu.py: no HIP, no GPU.
// stdin: one call per line, "name op=fwd|bwd|gq_fwd|gq_bwd key=value ...".  stdout: "name route" per line, the route as the kernel
// instantiations it launches with their grids and blocks.  Keys that are left out take the defaults below.
#include "../image2text_amd/csrc/attention_route.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

using namespace i2t;

static const char* tf(bool b) { return b ? "true" : "false"; }

// "<DROP,EVEN>" of a tiled kernel
static std::string variant(AttnDrop d) { return std::string("<") + tf(d != AttnDrop::None) + "," + tf(d != AttnDrop::Odd) + ">"; }

static std::string launch(const std::string& kernel, int grid, int block) {
    char b[64];
    snprintf(b, sizeof b, " grid=%d block=%d", grid, block);
    return kernel + b;
}

std::string attn_fwd_text(const AttnCall& c, const AttnKnobs& k) {
    const AttnFwdRoute r = attn_fwd_route(c, k);
    if (r.kind == AttnFwdKind::Fwd2)
        return launch(std::string("attn_fwd2_kernel<") + tf(r.drop != AttnDrop::None) + "," + std::to_string(r.per) + ">", r.grid, r.block);
    return launch("attn_fwd_kernel" + variant(r.drop), r.grid, r.block);
}

std::string attn_bwd_text(const AttnCall& c, const AttnKnobs& k) {
    const AttnBwdRoute r = attn_bwd_route(c, k);
    if (!r.q_seq_ok) return "refused out_drop_q_seq";
    const char* drop = tf(r.drop != AttnDrop::None);
    switch (r.kind) {
    case AttnBwdKind::Bwd3:
        return launch(std::string("attn_bwd3_kernel<") + drop + "," + std::to_string(r.nwv) + ">", r.grid, r.block) + " q_seq=" + std::to_string(r.q_seq);
    case AttnBwdKind::Bwd2: return launch(std::string("attn_bwd2_kernel<") + drop + ">", r.grid, r.block);
    case AttnBwdKind::Bwd1: return launch("attn_bwd1_kernel" + variant(r.drop), r.grid, r.block);
    case AttnBwdKind::Pair: break;
    }
    return launch("attn_bwd_dq_kernel" + variant(r.drop), r.grid, r.block) + " + " + launch("attn_bwd_dkv_kernel" + variant(r.drop), r.grid_dkv, r.block);
}

std::string gq_text(const AttnCall& c, bool backward) {
    const GqRoute r = gq_route(c);
    const std::string targs = "<" + std::to_string(r.d) + "," + tf(r.drop) + ">";
    if (!backward) return launch("gattn_fwd_kernel" + targs, r.grid_q, r.block);
    return launch("gattn_bwd_dq_kernel" + targs, r.grid_q, r.block) + " + " + launch("gattn_bwd_dkv_kernel" + targs, r.grid_dkv, r.block);
}

int main() {
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
        auto text = [&](const char* key, const char* dflt) { auto it = v.find(key); if (it == v.end()) return std::string(dflt); std::string x = it->second; v.erase(it); return x; };
        auto get = [&](const char* key, long dflt) { auto it = v.find(key); if (it == v.end()) return dflt; long x = atol(it->second.c_str()); v.erase(it); return x; };
        const std::string op = text("op", "fwd");
        const bool gq = op == "gq_fwd" || op == "gq_bwd";
        AttnCall c{};
        c.B = (int)get("B", 1); c.H = (int)get("H", 1); c.Hkv = (int)get("Hkv", c.H); c.hd = (int)get("hd", 64);
        c.Tq = (int)get("Tq", 64); c.Tk = (int)get("Tk", c.Tq); c.causal = (int)get("causal", 0);
        c.packed = get("packed", 0) != 0; c.drop = get("drop", 0) != 0; c.out_drop = get("od", 0) != 0;
        c.out_drop_q_seq = (int)get("q_seq", 0); c.split = (int)get("split", 0);
        AttnKnobs k{};
        k.v2 = get("v2", 1) != 0; k.bwd = (int)get("bwd", 3); k.bwd2 = get("bwd2", 1) != 0; k.bwd1 = get("bwd1", 1) != 0;
        k.bwd3_waves = (int)get("waves", 0);
        if (!v.empty()) { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), v.begin()->first.c_str()); return 2; }
        if (op != "fwd" && op != "bwd" && !gq) { fprintf(stderr, "%s: unknown op %s\n", name.c_str(), op.c_str()); return 2; }
        const std::string route = gq ? gq_text(c, op == "gq_bwd") : op == "fwd" ? attn_fwd_text(c, k) : attn_bwd_text(c, k);
        printf("%s %s\n", name.c_str(), route.c_str());
    }
    return 0;
}
