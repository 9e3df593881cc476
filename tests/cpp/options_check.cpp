// csrc/options.hpp on its own (no HIP): for every cdfem_set_option key, on a default Options, the default,
// the accepted values (the smallest and largest, or each listed one) stored in the right member and in no
// other, and the nearest refused values leaving everything unchanged and returning exactly the refusal's
// text.  The expectations below are written out by hand from the else-if ladder cdfem_set_option was before
// the table (commit 9a6263b); nothing here is generated from the table under test.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "options.hpp"

using namespace cdfem;

static int fails = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAIL line %d (%s): %s\n", __LINE__, what.c_str(), #cond); ++fails; } \
    } while (0)

struct Expect {
    const char *key;
    long long (*get)(const Options &);
    long long def;
    std::vector<int> accepted;
    std::vector<int> refused;
    std::string text;
    long long (*stored)(int);  // what an accepted value leaves in the member (null: the value)
};

#define GET(m) [](const Options &o) -> long long { return (long long)o.m; }
#define FLAG(k, d) {#k, GET(k), d, {0, 1}, {-1, 2}, #k " must be 0 or 1", nullptr}

static const std::vector<Expect> kExpect = {
    FLAG(brick_xcd, 1),
    {"brick_byte_limit", GET(brick_limit), 1LL << 31, {0, 1, 4096, INT_MAX}, {-1, INT_MIN},
     "brick_byte_limit must be 0 (the default 2^31) or 1..2^31-1", [](int v) -> long long { return v == 0 ? 1LL << 31 : v; }},
    {"den_group", GET(den_group_opt), 0, {0, 1, 2, 4, 8, 16, 32, 64}, {-1, 3, 63, 65, 128},
     "den_group must be 0 (automatic) or a power of two up to 64", nullptr},
    FLAG(cg_mr_fold, 1),
    FLAG(ho_brick_mfma, 0),
    {"brick_stagger", GET(brick_stagger), -1, {-1, 0, 511}, {-2, 512},
     "brick_stagger must be -1 (automatic), 0 (off) or 1..511", nullptr},
    FLAG(pa_uniform, 1),
    FLAG(pa_uniform_diag, 1),
    FLAG(ho_uniform, 0),
    {"ho_uniform_grid", GET(ho_uniform_grid), 0, {0, 1, INT_MAX}, {-1, INT_MIN},
     "ho_uniform_grid must be 0 (automatic) or the number of workgroups", nullptr},
    FLAG(brick_mfma, 0),
    {"ho_block_z", GET(ho_block_z), 2, {2, 4}, {1, 3, 5, 0}, "ho_block_z must be 2 or 4", nullptr},
    FLAG(ho_brick, 1),
    FLAG(mr_overlap, 1),
    FLAG(brick_mult_pb, 1),
    FLAG(cg_beta_fold, 1),
    FLAG(cg_beta_sum, 0),
    {"cg_den_fold", GET(cg_den_fold), 1024, {0, 64, 16384}, {-1, 1, 63, 16385}, "cg_den_fold must be 0 or 64..16384",
     nullptr},
    FLAG(brick_upd_pb, 1),
    FLAG(ho_dfold, 1),
    {"ho_mfma", GET(ho_mfma), 0, {0, 1, 3, 8, 9, 15}, {-1, 2, 4, 7, 10, 14, 16}, "ho_mfma must be 0, 1, 3, 8, 9 or 15",
     nullptr},
    FLAG(cg_xfold, 1),
    FLAG(cg_fused, 1),
    {"sell_order", GET(sell_mode), 8, {0, 8}, {-1, 9},
     "sell_order must be 0..8 (0 natural, 1 natural + windows, 2 RCM + windows, 3 auto, 4 RCM, 5 geometric, "
     "6 Morton + windows, 7 Morton, 8 Morton LDS windows / auto)",
     nullptr},
    {"gm_poll", GET(gm_poll), 4, {1, 64}, {0, 65, -1}, "gm_poll must be 1..64", nullptr},
    FLAG(gm_pb, 1),
    {"pa_affine", GET(pa_affine), 2, {0, 1, 2}, {-1, 3}, "pa_affine must be 0, 1 or 2", nullptr},
    FLAG(pa_geom, 0),
    FLAG(ho_geom, 0),
    {"spmv_lpr", GET(spmv_lpr), 0, {0, 1, 2, 4}, {-1, 3, 5, 8}, "spmv_lpr must be 0 (auto), 1, 2 or 4", nullptr},
    {"spmv_lds", GET(spmv_lds), -1, {-1, 0, 64, 65536}, {-2, 1, 63, 65, 65600},
     "spmv_lds must be -1 (auto), 0 (off) or rows per window, a multiple of 64 up to 65536", nullptr},
    {"sell_window", GET(sell_window), 0, {0, 64, 1 << 20}, {-1, 1, 63, 65, (1 << 20) + 64},
     "sell_window must be 0 (auto) or a multiple of 64 up to 2^20", nullptr},
    {"gm_ept", GET(gm_ept), 0, {0, 4, 5, 6, 8}, {-1, 1, 3, 7, 9}, "gm_ept must be 0 (auto), 4, 5, 6 or 8", nullptr},
    FLAG(spmv_xcd, 1),
    FLAG(spmv_index16, 1),
    {"profile_mask", GET(prof_mask), 0xFFFFFFFFLL, {INT_MIN, -1, 0, 5, INT_MAX}, {}, "",
     [](int v) -> long long { return (long long)(unsigned)v; }},
};

// every member but e's own still holds its default
static void others_untouched(const Options &o, const Expect &e, const std::string &what)
{
    for (const Expect &x : kExpect)
        if (x.get != e.get && std::string(x.key) != e.key) CHECK(x.get(o) == x.def);
}

int main()
{
    std::string what = "table";
    CHECK(kExpect.size() == 36);
    CHECK(sizeof(kOptionTable) / sizeof(kOptionTable[0]) == 36);
    for (const Expect &e : kExpect) {
        what = e.key;
        CHECK(e.get(Options{}) == e.def);
        for (int v : e.accepted) {
            what = std::string(e.key) + " = " + std::to_string(v);
            Options o;
            CHECK(set_option(o, e.key, v).empty());
            CHECK(e.get(o) == (e.stored ? e.stored(v) : (long long)v));
            others_untouched(o, e, what);
        }
        for (int v : e.refused) {
            what = std::string(e.key) + " = " + std::to_string(v);
            Options o;
            CHECK(set_option(o, e.key, v) == e.text);
            CHECK(e.get(o) == e.def);
            others_untouched(o, e, what);
            // and after an accepted value: the refusal keeps it
            CHECK(set_option(o, e.key, e.accepted.back()).empty());
            const long long kept = e.get(o);
            CHECK(set_option(o, e.key, v) == e.text);
            CHECK(e.get(o) == kept);
        }
    }
    what = "unknown and null keys";
    Options o;
    CHECK(set_option(o, "no_such_option", 1) == "unknown option no_such_option");
    CHECK(set_option(o, "", 1) == "unknown option ");
    CHECK(set_option(o, "brick_xc", 1) == "unknown option brick_xc");
    CHECK(set_option(o, "brick_xcd ", 1) == "unknown option brick_xcd ");
    CHECK(set_option(o, "den_group_opt", 1) == "unknown option den_group_opt");  // the member's name is not the key
    CHECK(set_option(o, nullptr, 1) == "key is null");
    for (const Expect &x : kExpect) CHECK(x.get(o) == x.def);
    if (fails == 0) std::printf("options ok\n");
    return fails != 0;
}
