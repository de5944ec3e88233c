// Prints the answers of the dispatch plan (csrc/scvote_plan.h, the library's own code: plain C++, no HIP) on the CPU: built and run by
// tests/test_dispatch_plan_cpu.py, which states what every answer must be.  Reads queries from standard input, one per line, and prints one
// line of integers per query:
//   opt KEY VALUE       set a field of the options (until `reset`); prints nothing
//   reset               the defaults of scv_create on an MI355X (256 CUs, 160 KiB of LDS)
//   <query> ARGS...     see the table in main()
// g++ -std=c++17 -o plan_check plan_check.cpp; also built with -fsanitize=address,undefined (nothing here allocates or shifts out of range).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../o1_inference_scaling_laws_amd/csrc/scvote_plan.h"

using namespace scv::plan;

static Options defaults() { return Options{0, 0, 32, 8192, 64, 8, 0, 512, 0, 0, 256, 16, 1024, 1, 4, false, 256, 160 * 1024}; }

static bool set_opt(Options& o, const std::string& k, long long v) {
#define F(name) if (k == #name) { o.name = (decltype(o.name))v; return true; }
    F(path) F(prefix_path) F(tiny_n_max) F(reg_n_max) F(sort_n_max) F(sort_n_min) F(reg_shape) F(fused_counters_max) F(overwrite_counters)
    F(segs_override) F(split_seg_kb) F(copies) F(threads) F(wg_per_cu) F(unroll) F(user_tuned) F(num_cus) F(lds_max)
#undef F
    return false;
}

int main() {
    Options o = defaults();
    static const char* kinds[] = {"LANE", "SORT", "REG", "STREAM"};
    static const char* forms[] = {"POOL", "CELLS", "LANE", "HIST"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        if (!(in >> q) || q[0] == '#') continue;
        if (q == "reset") { o = defaults(); continue; }
        if (q == "opt") {
            std::string k; long long v;
            if (!(in >> k >> v) || !set_opt(o, k, v)) { fprintf(stderr, "bad option: %s\n", line.c_str()); return 2; }
            continue;
        }
        std::vector<long long> a;
        for (long long v; in >> v;) a.push_back(v);
        auto need = [&](size_t n) { if (a.size() != n) { fprintf(stderr, "bad query: %s\n", line.c_str()); exit(2); } };
        if (q == "nv") { need(1); printf("%d %d %d %d\n", lane_nv(a[0]), prefix_lane_nv(a[0]), sort_nv(a[0]), sort_prefix_nv(a[0])); }
        else if (q == "lanelds") { need(2); printf("%zu\n", lane_kernel_lds((int32_t)a[0], (int)a[1])); }
        else if (q == "kind") { need(5); printf("%s\n", kinds[cell_kind(o, a[0], (int32_t)a[1], a[2] != 0, a[3] != 0, a[4] != 0)]); }     // N B rows_aligned tok pool_rows
        else if (q == "sortfb") { need(2); printf("%s\n", kinds[sort_fallback_kind(o, a[0], (int32_t)a[1])]); }                             // N B
        else if (q == "packed") { need(4); if (a[0] < 0 || a[0] > 3) { fprintf(stderr, "bad kind: %s\n", line.c_str()); return 2; } printf("%d\n", (int)packed_ok((Kind)a[0], RegShape{(int)a[1], (int)a[2], (int)a[3]})); }   // kind (0 LANE 1 SORT 2 REG 3 STREAM) g v h
        else if (q == "shape") { need(3); const RegShape s = reg_shape(a[0], (int)a[1], a[2] != 0); printf("%d %d %d\n", s.g, s.v, s.h); }      // Nreg forced have_g8
        else if (q == "reggrid") { need(4); printf("%lld\n", (long long)reg_grid(a[0], a[1], (int)a[2], (int32_t)a[3])); }                   // resident nbatches WPG B
        else if (q == "band") { need(2); const StreamBand b = stream_band(o, a[0], a[1]); printf("%d %d %d %d %zu\n", b.copies, b.threads, b.wg_per_cu, b.unroll, b.lds); }   // N ncells
        else if (q == "split") { need(3); const Split s = split(o, a[0], a[1], a[2]); printf("%lld %lld\n", (long long)s.S, (long long)s.seg_len); }   // N ncells slots
        else if (q == "grid") { need(3); printf("%lld\n", (long long)stream_grid(a[0], a[1], (int)a[2])); }                                  // nitems slots grid_override
        else if (q == "disp") { need(3); printf("%d\n", (int)use_dispenser(o, a[0], a[1], a[2])); }                                          // nitems grid item_len
        else if (q == "tcl") { need(3); printf("%lld\n", (long long)lds_tie_classes(a[0], (int32_t)a[1], a[2])); }                           // spare_words B N
        else if (q == "chunks") { need(2); printf("%lld\n", (long long)reduce_chunks(a[0], (int32_t)a[1], o.num_cus)); }                     // P B
        else if (q == "reduce") { need(5); printf("%d\n", (int)counters_by_reduce(o, a[0] != 0, a[1] != 0, a[2], (int32_t)a[3], a[4])); }   // want streaming ncells B N
        else if (q == "owfew") { need(3); printf("%d\n", (int)overwrite_few_cells(o, a[0] != 0, a[1], (int32_t)a[2])); }                     // want ncells B
        else if (q == "lanegrid") { need(4); printf("%lld\n", (long long)lane_grid(o, a[0], (int)a[1], a[2] != 0, (int32_t)a[3])); }          // ncells nv tok B
        else if (q == "tclds") { need(2); printf("%zu\n", tie_classes_lds((int32_t)a[0], a[1])); }                                          // B tcl
        else if (q == "nvc") { need(2); printf("%lld\n", (long long)nv_cache_words(a[0] != 0, (int32_t)a[1])); }                            // has_n_valid B
        else if (q == "bgrid") { need(3); printf("%lld\n", (long long)b_multiple_grid(a[0], a[1], (int32_t)a[2])); }                         // grid cells_per_wg B
        else if (q == "few") { need(6); const FewVotes f = few_votes(o, a[0], (int32_t)a[1], a[2], a[3] != 0, a[4] != 0, (int)a[5]); printf("%d %d %lld\n", (int)f.ok, (int)f.one, (long long)f.grid); }   // N B ncells bases_aligned pool_rows grid_override
        else if (q == "sortw") {                                                                                                            // waves N tok lin has_n_valid B
            need(6);
            const int64_t region = sort_region_words(a[1], a[2] != 0, a[3] != 0), tail = sort_tail_words(a[4] != 0, (int32_t)a[5], sort_nv(a[1]));
            printf("%lld %lld %d\n", (long long)region, (long long)tail, sort_waves((int)a[0], region, tail, o.lds_max));
        }
        else if (q == "spw") { need(3); const int64_t region = sort_prefix_region_words(a[1], sort_prefix_nv(a[1])); printf("%lld %d\n", (long long)region, sort_prefix_waves((int)a[0], region, a[2], o.lds_max)); }   // waves N tail_words
        else if (q == "rows") { need(3); printf("%d\n", (int)pool_rows_eligible(o, (int32_t)a[0], a[1], a[2] != 0)); }                        // B N rows_aligned
        else if (q == "plane") { need(3); const PrefixLane l = prefix_lane(o, (int32_t)a[0], a[1], a[2] != 0); printf("%d %d %d %zu %zu\n", (int)l.ok, l.nv, l.threads, l.lds, l.lds_total); }   // B N tok
        else if (q == "served") { need(2); printf("%d\n", (int)budget_served(a[0], a[1])); }                                                 // n N
        else if (q == "spe") { need(4); printf("%d\n", (int)sort_prefix_eligible(o, a[0], (int32_t)a[1], a[2], a[3] != 0)); }                // P B N rows_aligned
        else if (q == "form") { need(5); printf("%s\n", forms[prefix_form(o, (int32_t)a[0], a[1], a[2] != 0, a[3] != 0, a[4] != 0)]); }      // B N rows_aligned lane_fits skip_sortable
        else if (q == "ppl") { need(2); printf("%d\n", prefix_pool_lanes(o, a[0], a[1] != 0)); }                                             // N rows_aligned
        else { fprintf(stderr, "unknown query: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
