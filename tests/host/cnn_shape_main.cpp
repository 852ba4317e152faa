// tests/host/cnn_shape_main.cpp -- the shape and launch rules of simple_cnn (csrc/kws_cnn_shape.h, csrc/kws_cnn_plan.h) as a plain host
// program: it reads one query per line from stdin and answers each with one line of JSON.  It holds no case table of its own;
// tests/test_cnn_shape_host.py owns the cases and compares the answers with the Python restatements of the rules.
//
//   dims nf fs                                      the maps of kws_model_create
//   stage nf fs l                                   cnn_stage
//   pad n k s                                       same_out, same_pad_before
//   plan kind nf fs C head_K B mprec det capturing training wants_head prepared
//   dgrad B H W stride KH KW simds                  dgrad_plan (rc != 0: refused)
//   wgrad steps gy slots det                        wgrad_round
//   wgrad_bf16 nchunk ngroups slots det             wgrad_bf16_round
//   wgrad_pm B H W stride max_slots min_chunks      wgrad_pm_plan over a 3x3 'same' geometry (ok = false: refused)
//   stat M C                                        stat_grid
//   l1 B                                            l1_grid
//   even_grid B max_blocks
// An unknown or malformed query is answered with {"error": ...} and makes the exit status 1.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "kws_cnn_plan.h"

using namespace kws;

namespace {

template <typename... T>
bool read(std::istringstream &in, T &...v)
{
    return static_cast<bool>((in >> ... >> v));
}

void print_dims(const CnnDims &d)
{
    std::printf("{\"H0\": %d, \"W0\": %d, \"H1\": %d, \"W1\": %d, \"H2\": %d, \"W2\": %d, \"H3\": %d, \"W3\": %d, \"H4\": %d, \"W4\": %d, \"flat\": %d}\n",
                d.H0, d.W0, d.H1, d.W1, d.H2, d.W2, d.H3, d.W3, d.H4, d.W4, d.flat);
}

void print_plan(const CnnPlan &p)
{
    const struct { const char *name; bool on; } f[] = {
        {"training", p.training}, {"bf16", p.bf16}, {"det", p.det}, {"prepared", p.prepared}, {"fused_tail", p.fused_tail}, {"group", p.group},
        {"dense_fused", p.dense_fused}, {"l1m", p.l1m}, {"l1_default_map", p.l1_default_map}, {"prep_in_stats", p.prep_in_stats},
        {"l1_conv2", p.l1_conv2}, {"compact_g2", p.compact_g2}, {"routed_g2", p.routed_g2}, {"fuse_pool2", p.fuse_pool2}, {"acc_fwd", p.acc_fwd},
        {"acc_bn2", p.acc_bn2}, {"acc_bn3", p.acc_bn3}, {"acc_bn4", p.acc_bn4}, {"a3_on_load", p.a3_on_load}, {"pool4_fused", p.pool4_fused},
        {"wgrad_pmajor", p.wgrad_pmajor}, {"wgrad2_bf16", p.wgrad2_bf16}, {"wgrad2_early", p.wgrad2_early}, {"wgrad2_fast", p.wgrad2_fast},
        {"l1_fin_in_kernel", p.l1_fin_in_kernel}, {"head_bwd_fuses", p.head_bwd_fuses}, {"fuse_head_fwd", p.fuse_head_fwd}};
    const char *sep = "{";
    for (const auto &x : f) {
        std::printf("%s\"%s\": %s", sep, x.name, x.on ? "true" : "false");
        sep = ", ";
    }
    std::printf("}\n");
}

bool answer(const std::string &line)
{
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) return true;                    // an empty line
    if (what == "dims") {
        int nf, fs;
        if (!read(in, nf, fs)) return false;
        print_dims(cnn_dims(nf, fs));
    } else if (what == "stage") {
        int nf, fs, l;
        if (!read(in, nf, fs, l) || l < 0 || l > 3) return false;
        const CnnStage t = cnn_stage(cnn_dims(nf, fs), l);
        std::printf("{\"Hi\": %d, \"Wi\": %d, \"Ho\": %d, \"Wo\": %d, \"stride\": %d, \"Cin\": %d, \"Cout\": %d, \"pooled\": %s, \"relu\": %s}\n", t.Hi, t.Wi,
                    t.Ho, t.Wo, t.stride, t.Cin, t.Cout, t.pooled ? "true" : "false", t.relu ? "true" : "false");
    } else if (what == "pad") {
        int n, k, s;
        if (!read(in, n, k, s) || s < 1) return false;
        std::printf("{\"out\": %d, \"before\": %d}\n", same_out(n, s), same_pad_before(n, k, s));
    } else if (what == "plan") {
        int kind, nf, fs, C, head_K, B, mprec, det, capturing, training, wants_head, prepared;
        if (!read(in, kind, nf, fs, C, head_K, B, mprec, det, capturing, training, wants_head, prepared)) return false;
        const CnnDesc m{kind, C, head_K, det, cnn_dims(nf, fs)};
        print_plan(plan_cnn(m, B, mprec, training != 0, capturing != 0, wants_head != 0, prepared != 0));
    } else if (what == "dgrad") {
        ConvGeom g;
        long simds;
        if (!read(in, g.B, g.H, g.W, g.stride, g.KH, g.KW, simds) || g.stride < 1 || simds < 1) return false;
        g.Ho = same_out(g.H, g.stride); g.Wo = same_out(g.W, g.stride);
        g.pt = same_pad_before(g.H, g.KH, g.stride); g.pl = same_pad_before(g.W, g.KW, g.stride);
        DgradPlan p;
        const int rc = dgrad_plan(g, simds, p);
        if (rc != DGRAD_OK) {
            std::printf("{\"rc\": %d}\n", rc);
            return true;
        }
        std::printf("{\"rc\": 0, \"mw\": %d, \"max_rows\": %ld, \"classes\": [", p.mw, p.max_rows);
        for (int i = 0; i < p.ncls; ++i) {
            const DgradClass &c = p.cls.c[i];
            std::printf("%s[%d, %d, %d, %d]", i ? ", " : "", c.cy, c.cx, c.ny, c.nx);
        }
        std::printf("]}\n");
    } else if (what == "wgrad") {
        long steps, slots;
        int gy, det;
        if (!read(in, steps, gy, slots, det) || gy < 1) return false;
        const WgradRound r = wgrad_round(steps, gy, slots, det != 0);
        std::printf("{\"gx\": %ld, \"spw\": %d}\n", r.gx, r.spw);
    } else if (what == "wgrad_bf16") {
        long nchunk, slots;
        int ngroups, det;
        if (!read(in, nchunk, ngroups, slots, det) || ngroups < 1) return false;
        const WgradBf16Round r = wgrad_bf16_round(nchunk, ngroups, slots, det != 0);
        std::printf("{\"nranges\": %ld, \"cpb\": %d}\n", r.nranges, r.cpb);
    } else if (what == "wgrad_pm") {
        int B, H, W, stride, max_slots, min_chunks;
        if (!read(in, B, H, W, stride, max_slots, min_chunks) || stride < 1 || min_chunks < 1) return false;
        const ConvGeom g = geom3x3(B, H, W, stride);
        WgradPm pm{};
        if (!wgrad_pm_plan(g, max_slots, min_chunks, pm)) {
            std::printf("{\"ok\": false}\n");
            return true;
        }
        std::printf("{\"ok\": true, \"pos\": [");
        for (int tap = 0; tap < 9; ++tap) {
            std::printf("%s[", tap ? ", " : "");
            for (int i = 0; i < pm.npos[tap]; ++i) std::printf("%s%d", i ? ", " : "", (int)((pm.pos[tap] >> (4 * i)) & 15ull));
            std::printf("]");
        }
        std::printf("], \"npos\": [");
        for (int tap = 0; tap < 9; ++tap) std::printf("%s%d", tap ? ", " : "", pm.npos[tap]);
        std::printf("], \"slot0\": [");
        for (int tap = 0; tap < 10; ++tap) std::printf("%s%d", tap ? ", " : "", pm.slot0[tap]);
        std::printf("]}\n");
    } else if (what == "stat") {
        long M;
        int C, nblk, rows;
        if (!read(in, M, C) || M < 1 || C < 1 || C > 256) return false;
        stat_grid(M, C, nblk, rows);
        std::printf("{\"nblk\": %d, \"rows\": %d}\n", nblk, rows);
    } else if (what == "l1") {
        int B;
        if (!read(in, B)) return false;
        const L1Grid g = l1_grid(B);
        std::printf("{\"cpb\": %d, \"nb\": %d, \"cpw\": %d, \"nbm\": %d}\n", g.cpb, g.nb, g.cpw, g.nbm);
    } else if (what == "even_grid") {
        int B, max_blocks;
        if (!read(in, B, max_blocks) || B < 1 || max_blocks < 1) return false;
        std::printf("{\"grid\": %u}\n", even_grid(B, max_blocks));
    } else
        return false;
    return true;
}

}  // namespace

int main()
{
    int status = 0;
    std::string line;
    while (std::getline(std::cin, line))
        if (!answer(line)) {
            std::printf("{\"error\": \"unknown or malformed query\"}\n");
            status = 1;
        }
    return status;
}
