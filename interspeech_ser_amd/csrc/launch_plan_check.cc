// Prints the launch plans of launch_plan.h (`make plan_check`: plain g++ on this file + hosterr.hip, no GPU and no HIP header).
// Test infrastructure: tests/test_launch_plan_host.py feeds it the case list and compares with tests/golden/launch_plans.txt.
//
// stdin, one case per line:   gemm FIELD=VALUE ...   |   attn FIELD=VALUE ...
//   FIELD is a member of ser_gemm_args / ser_attention_args; members not named are zero.  A pointer member takes 0 or 1 (1 = a dummy
//   non-null address; nothing is dereferenced).
// stdout, one line per case:
//   gemm <tile> <MODE>><OM> grid=<x>x<y> block=<threads> lds=<bytes>
//   attn <dhp> <mode> <PTBGO> nbuf=.. bias_stride=.. lds=.. grid=..      (a letter of PRE, TBL, B2D, GB, OCC where the flag is set, else '-')
//   gemm err <code>   |   attn err <code>
// With the argument --epi a gemm line also ends in ` epi=<class>`, the epilogue class of the launch (GEMM_EPI_NAME).
#include "launch_plan.h"
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>

enum kind { I32, I64, F32, PTR };
struct field { const char* name; size_t off; kind k; };
#define F(S, M, K) {#M, offsetof(S, M), K}
static const field GEMM_FIELDS[] = {
    F(ser_gemm_args, A, PTR), F(ser_gemm_args, a_rowoff, PTR), F(ser_gemm_args, lda, I64), F(ser_gemm_args, kc, I32), F(ser_gemm_args, W, PTR),
    F(ser_gemm_args, M, I32), F(ser_gemm_args, N, I32), F(ser_gemm_args, K, I32), F(ser_gemm_args, groups, I32),
    F(ser_gemm_args, c_group_stride, I32), F(ser_gemm_args, mode, I32), F(ser_gemm_args, act, I32), F(ser_gemm_args, residual, PTR),
    F(ser_gemm_args, ldr, I64), F(ser_gemm_args, out_f32, PTR), F(ser_gemm_args, ldo_f32, I64), F(ser_gemm_args, out_act, PTR),
    F(ser_gemm_args, ldo_act, I64), F(ser_gemm_args, ln_gamma, PTR), F(ser_gemm_args, ln_beta, PTR), F(ser_gemm_args, tile_cfg, I32),
    F(ser_gemm_args, ln_stats_in, PTR), F(ser_gemm_args, ln_groups, I32), F(ser_gemm_args, ln_colsum, PTR), F(ser_gemm_args, stat_out, PTR),
    F(ser_gemm_args, stat_groups, I32), F(ser_gemm_args, f32_col_begin, I32), F(ser_gemm_args, col_scale_end, I32),
    F(ser_gemm_args, shift_out, PTR), F(ser_gemm_args, out_mode, I32), F(ser_gemm_args, mean_out, PTR), F(ser_gemm_args, lnstat_out, PTR),
    F(ser_gemm_args, a_scale, PTR), F(ser_gemm_args, a_scale_ld, I64), F(ser_gemm_args, w_scale, PTR), F(ser_gemm_args, w_scale_ld, I64),
    F(ser_gemm_args, out_scale, PTR), F(ser_gemm_args, gn_scale, PTR), F(ser_gemm_args, gn_shift, PTR), F(ser_gemm_args, gn_row_offs, PTR),
    F(ser_gemm_args, gn_B, I32), F(ser_gemm_args, gn_ld, I32),
};
static const field ATTN_FIELDS[] = {
    F(ser_attention_args, qkv, PTR), F(ser_attention_args, ld, I64), F(ser_attention_args, q_col, I32), F(ser_attention_args, k_col, I32),
    F(ser_attention_args, v_col, I32), F(ser_attention_args, B, I32), F(ser_attention_args, frame_offs, PTR), F(ser_attention_args, table, PTR),
    F(ser_attention_args, gate, PTR), F(ser_attention_args, max_frames, I32), F(ser_attention_args, table_T, I32), F(ser_attention_args, out, PTR),
    F(ser_attention_args, ldo, I64), F(ser_attention_args, H, I32), F(ser_attention_args, dh, I32), F(ser_attention_args, scale, F32),
    F(ser_attention_args, mode, I32), F(ser_attention_args, gate_col, I32), F(ser_attention_args, out_mode, I32),
    F(ser_attention_args, gru_const, PTR), F(ser_attention_args, key_lens, PTR), F(ser_attention_args, bias2d, PTR),
    F(ser_attention_args, bias2d_ld, I64), F(ser_attention_args, gate_x, PTR), F(ser_attention_args, gate_x_ld, I64),
    F(ser_attention_args, gate_x_plane_stride, I64), F(ser_attention_args, gate_stat, PTR), F(ser_attention_args, gate_w, PTR),
    F(ser_attention_args, gate_cb, PTR), F(ser_attention_args, gate_x_planes, I32), F(ser_attention_args, gate_w_plane_stride, I64),
    F(ser_attention_args, out_scale, PTR), F(ser_attention_args, out_scale_ld, I64),
};
#undef F

static char g_dummy[16];

template <size_t N>
static bool parse(std::istringstream& in, void* args, const field (&fields)[N]) {
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        const std::string name = tok.substr(0, eq), val = tok.substr(eq + 1);
        const field* f = nullptr;
        for (const field& c : fields)
            if (name == c.name) f = &c;
        if (!f) return false;
        char* dst = (char*)args + f->off;
        switch (f->k) {
            case I32: { const int32_t v = (int32_t)strtol(val.c_str(), nullptr, 10); memcpy(dst, &v, sizeof(v)); break; }
            case I64: { const int64_t v = (int64_t)strtoll(val.c_str(), nullptr, 10); memcpy(dst, &v, sizeof(v)); break; }
            case F32: { const float v = strtof(val.c_str(), nullptr); memcpy(dst, &v, sizeof(v)); break; }
            case PTR: { const void* v = val == "0" ? nullptr : g_dummy; memcpy(dst, &v, sizeof(v)); break; }
        }
    }
    return true;
}

int main(int argc, char** argv) {
    const bool show_epi = argc > 1 && !strcmp(argv[1], "--epi");
    std::string line;
    int lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        bool ok = false;
        if (what == "gemm") {
            ser_gemm_args a = {};
            gemm_launch pl = {};
            if ((ok = parse(in, &a, GEMM_FIELDS))) {
                const int rc = gemm_plan(&a, &pl);
                if (rc) printf("gemm err %d\n", rc);
                else {
                    printf("gemm %s %d>%d grid=%ux%u block=%d lds=%d", GEMM_TILE[pl.tile].name, GEMM_PAIR[pl.pair].mode, GEMM_PAIR[pl.pair].om,
                           pl.grid_x, pl.grid_y, pl.block, pl.lds);
                    printf(show_epi ? " epi=%s\n" : "\n", GEMM_EPI_NAME[pl.epi]);
                }
            }
        } else if (what == "attn") {
            ser_attention_args a = {};
            attn_launch pl = {};
            if ((ok = parse(in, &a, ATTN_FIELDS))) {
                const int rc = attn_plan(&a, &pl);
                if (rc) printf("attn err %d\n", rc);
                else printf("attn %d %d %c%c%c%c%c nbuf=%d bias_stride=%d lds=%zu grid=%u\n", pl.dhp, pl.mode, pl.pre ? 'P' : '-', pl.tbl ? 'T' : '-',
                            pl.b2d ? 'B' : '-', pl.gb ? 'G' : '-', pl.occ ? 'O' : '-', pl.nbuf, pl.bias_stride, pl.lds, pl.grid);
            }
        }
        if (!ok) {
            fprintf(stderr, "launch_plan_check: cannot read line %d: %s\n", lineno, line.c_str());
            return 2;
        }
    }
    return 0;
}
