// sweep_tables_host.cpp -- the two tables of the sweep's host side (x264_vs2008_amd/csrc/sweep_tables.h) and their walks, compiled for
// the host alone (tests/test_cpu_sweep_tables.py builds it with -fsanitize=address,undefined and runs it).  The launch functions are
// stand-ins that record what they were asked to launch; what the walks are held to is the arithmetic they replaced, restated here.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "x264hip.h"

#define SW_MAX_REFS 8
struct SwArgs { int x; };
struct SwRefs { int x; };
struct SwRd { int x; };
struct SwDesc { int kind; };                          // an entry remembers the kind it was built as
typedef struct ihipStream_t *hipStream_t;
#include "sweep_tables.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Launch { std::string fn; long at; int n; hipStream_t stream; };
static std::vector<Launch> launched;
static const SwDesc *table;
#define FRAME_STUB(name) void name(const SwArgs &, const SwRefs &, const SwRd &, hipStream_t s) { launched.push_back({#name, -1, 0, s}); }
#define CHAINS_STUB(name) void name(const SwDesc *tab, int n, hipStream_t s) { launched.push_back({#name, (long)(tab - table), n, s}); }
FRAME_STUB(x264hip_launch_slice_rd) FRAME_STUB(x264hip_launch_slice_rf) FRAME_STUB(x264hip_launch_slice_ll)
FRAME_STUB(x264hip_launch_slice_ll_rf) FRAME_STUB(x264hip_launch_slice_b) FRAME_STUB(x264hip_launch_slice_bt)
CHAINS_STUB(x264hip_launch_slice_rd_ch) CHAINS_STUB(x264hip_launch_slice_rf_ch) CHAINS_STUB(x264hip_launch_slice_ll_ch)
CHAINS_STUB(x264hip_launch_slice_ll_rf_ch) CHAINS_STUB(x264hip_launch_slice_bt_ch)

// ---- the arrays of the state: the list x264hip_mb_state_alloc_ex held before the table (member, bytes for n macroblocks)
static void check_state_arrays()
{
    const int mb_w = 5, mb_h = 3, batch = 2;
    const size_t n = (size_t)mb_w * mb_h * batch;
    x264hip_mb_state s, *st = &s;
    memset(st, 0, sizeof(*st));
    struct { void **p; size_t bytes; } items[] = {
        {(void **)&st->mb_type, n}, {(void **)&st->partition, n}, {(void **)&st->sub_partition, 4 * n}, {(void **)&st->ref, 4 * n}, {(void **)&st->i4mode, 16 * n},
        {(void **)&st->i16mode, n}, {(void **)&st->chroma_mode, n}, {(void **)&st->qp, n}, {(void **)&st->t8, n},
        {(void **)&st->mv, 64 * n}, {(void **)&st->mvr, 4 * SW_MAX_REFS * n}, {(void **)&st->cbp, 2 * n}, {(void **)&st->nnz, 27 * n},
        {(void **)&st->luma, 512 * n}, {(void **)&st->luma_dc, 32 * n}, {(void **)&st->chroma_dc, 16 * n}, {(void **)&st->chroma_ac, 256 * n},
        {(void **)&st->cost_intra, 4 * n}, {(void **)&st->cost_inter, 4 * n}, {(void **)&st->cost_intra_alt, 4 * n},
        {(void **)&st->progress, sizeof(int) * ((size_t)mb_h * batch + 1)}, {(void **)&st->mvd, 64 * n},
        {(void **)&st->mv1, 64 * n}, {(void **)&st->ref1, 4 * n}, {(void **)&st->mvr1, 4 * n}, {(void **)&st->mvd1, 64 * n}, {(void **)&st->skipbp, n}};
    const size_t n_items = sizeof(items) / sizeof(items[0]), n_rows = sizeof(k_state_arrays) / sizeof(k_state_arrays[0]);
    CHECK(n_rows == n_items, "%zu rows, %zu arrays", n_rows, n_items);
    size_t level_bytes = 0, all_bytes = 0;
    for (size_t i = 0; i < n_rows && i < n_items; i++) {
        const StateArray &row = k_state_arrays[i];
        CHECK(state_array(st, row) == items[i].p, "row %zu is not array %zu of the allocation order", i, i);
        CHECK(state_array_bytes(row, mb_w, mb_h, batch) == items[i].bytes, "row %zu: %zu bytes, not %zu", i, state_array_bytes(row, mb_w, mb_h, batch), items[i].bytes);
        const bool level = items[i].p == (void **)&st->luma || items[i].p == (void **)&st->luma_dc || items[i].p == (void **)&st->chroma_dc || items[i].p == (void **)&st->chroma_ac;
        CHECK(row.level == level, "row %zu: level array %d", i, (int)row.level);
        if (row.mb_bytes) { all_bytes += row.mb_bytes; level_bytes += row.level ? row.mb_bytes : 0; }
    }
    CHECK(all_bytes == 1184 && level_bytes == 816, "%zu bytes per macroblock, %zu of them levels", all_bytes, level_bytes);
    // every pointer of the structure exactly once: written through the table, each member reads back its own row's mark, and what is
    // left of the structure is its scalars (poc, n_ref0, inv_ref_poc[8], ref_poc[8])
    static char marks[64];
    for (size_t i = 0; i < n_rows; i++) {
        CHECK(k_state_arrays[i].member % sizeof(void *) == 0 && k_state_arrays[i].member + sizeof(void *) <= sizeof(*st), "row %zu: offset %zu", i, k_state_arrays[i].member);
        CHECK(*state_array(st, k_state_arrays[i]) == nullptr, "row %zu names a member an earlier row named", i);
        *state_array(st, k_state_arrays[i]) = marks + i;
    }
    for (size_t i = 0; i < n_items; i++) CHECK(*items[i].p == marks + i, "array %zu is in no row", i);
    CHECK(sizeof(*st) == n_rows * sizeof(void *) + 18 * sizeof(int), "x264hip_mb_state has a member that is neither in the table nor a known scalar");
    CHECK(state_progress_bytes(mb_h, batch) == sizeof(int) * ((size_t)mb_h * batch + 1), "progress bytes");
}

// ---- the kinds: for cnt_in[k] entries built as kind k, the sorted table and the launches against the arithmetic of the `if` chain
static void check_kinds(const int cnt_in[SW_N_KINDS], bool two)
{
    // build pass: entries in a kind-interleaved order, so that placement has something to sort
    std::vector<int> kinds;
    for (int round = 0; round < 2; round++)
        for (int k = SW_N_KINDS - 1; k >= 0; k--) if (cnt_in[k] > round) kinds.push_back(k);
    const int n = (int)kinds.size();
    int cnt[SW_N_KINDS] = {0};
    std::vector<SwDesc> tmp((size_t)n), got((size_t)n + 1), want((size_t)n + 1);
    for (int i = 0; i < n; i++) {
        tmp[i].kind = kinds[i];
        int want_kind = kinds[i];
        if (want_kind == SW_KIND_B) want_kind = SW_KIND_BT;                       // one B kernel in the table launches
        kinds[i] = k_sweep_kinds[kinds[i]].in_table;
        CHECK(kinds[i] == want_kind, "kind %d becomes %d in a table", tmp[i].kind, kinds[i]);
        cnt[kinds[i]]++;
    }
    const int n_ll = cnt[SW_KIND_LL] + cnt[SW_KIND_LL_RF];
    if (n_ll && n_ll != n) return;                      // refused before anything is placed: a table is all-lossless or not at all
    // the walk
    int base[SW_N_KINDS], at[SW_N_KINDS];
    sweep_place(cnt, base);
    memcpy(at, base, sizeof(at));
    for (int i = 0; i < n; i++) { CHECK(at[kinds[i]] < n, "placement past the table"); if (at[kinds[i]] < n) got[at[kinds[i]]++] = tmp[i]; }
    // what it replaced
    int wbase[SW_N_KINDS] = {0}, wat[SW_N_KINDS];
    wbase[SW_KIND_RD] = 0; wbase[SW_KIND_RF] = cnt[SW_KIND_RD]; wbase[SW_KIND_BT] = wbase[SW_KIND_RF] + cnt[SW_KIND_RF];
    wbase[SW_KIND_LL] = 0; wbase[SW_KIND_LL_RF] = cnt[SW_KIND_LL];
    for (int k = 0; k < SW_N_KINDS; k++) wat[k] = wbase[k];
    for (int i = 0; i < n; i++) want[wat[kinds[i]]++] = tmp[i];
    for (int i = 0; i < n; i++) CHECK(got[i].kind == want[i].kind, "entry %d of the sorted table is of kind %d, not %d", i, got[i].kind, want[i].kind);
    hipStream_t s = (hipStream_t)&failures, sb = two ? (hipStream_t)&table : s;
    table = got.data();
    launched.clear();
    sweep_enqueue(table, cnt, base, s, sb);
    std::vector<Launch> w;
    if (cnt[SW_KIND_RD]) w.push_back({"x264hip_launch_slice_rd_ch", wbase[SW_KIND_RD], cnt[SW_KIND_RD], s});
    if (cnt[SW_KIND_RF]) w.push_back({"x264hip_launch_slice_rf_ch", wbase[SW_KIND_RF], cnt[SW_KIND_RF], s});
    if (cnt[SW_KIND_LL]) w.push_back({"x264hip_launch_slice_ll_ch", wbase[SW_KIND_LL], cnt[SW_KIND_LL], s});
    if (cnt[SW_KIND_LL_RF]) w.push_back({"x264hip_launch_slice_ll_rf_ch", wbase[SW_KIND_LL_RF], cnt[SW_KIND_LL_RF], s});
    if (cnt[SW_KIND_BT]) w.push_back({"x264hip_launch_slice_bt_ch", wbase[SW_KIND_BT], cnt[SW_KIND_BT], sb});
    CHECK(launched.size() == w.size(), "%zu launches, not %zu", launched.size(), w.size());
    for (size_t i = 0; i < launched.size() && i < w.size(); i++)
        CHECK(launched[i].fn == w[i].fn && launched[i].at == w[i].at && launched[i].n == w[i].n && launched[i].stream == w[i].stream,
              "launch %zu: %s at %ld, %d entries; expected %s at %ld, %d entries (or the other stream)", i, launched[i].fn.c_str(), launched[i].at, launched[i].n,
              w[i].fn.c_str(), w[i].at, w[i].n);
}

int main()
{
    check_state_arrays();
    // the lock-step launch of every kind: the `switch` it replaced
    const char *frame_fn[SW_N_KINDS] = {nullptr};
    frame_fn[SW_KIND_RD] = "x264hip_launch_slice_rd"; frame_fn[SW_KIND_RF] = "x264hip_launch_slice_rf"; frame_fn[SW_KIND_LL] = "x264hip_launch_slice_ll";
    frame_fn[SW_KIND_LL_RF] = "x264hip_launch_slice_ll_rf"; frame_fn[SW_KIND_B] = "x264hip_launch_slice_b"; frame_fn[SW_KIND_BT] = "x264hip_launch_slice_bt";
    for (int k = 0; k < SW_N_KINDS; k++) {
        CHECK((k_sweep_kinds[k].frame != nullptr) == (frame_fn[k] != nullptr), "kind %d: lock-step launch", k);
        if (!k_sweep_kinds[k].frame || !frame_fn[k]) continue;
        launched.clear();
        k_sweep_kinds[k].frame(SwArgs(), SwRefs(), SwRd(), nullptr);
        CHECK(launched.size() == 1 && launched[0].fn == frame_fn[k], "kind %d launches %s", k, launched.empty() ? "nothing" : launched[0].fn.c_str());
    }
    // every mix of 0..2 entries of every kind a chain table can hold (PLAIN is refused: the table belongs to the raster variant)
    int cnt[SW_N_KINDS], mixes = 0;
    for (int code = 0; code < 729; code++) {
        cnt[SW_KIND_PLAIN] = 0;
        for (int k = 1, c = code; k < SW_N_KINDS; k++, c /= 3) cnt[k] = c % 3;
        for (int two = 0; two < 2; two++) check_kinds(cnt, two != 0);
        mixes++;
    }
    printf("%d mixes, %d failures\n", mixes, failures);
    return failures != 0;
}
