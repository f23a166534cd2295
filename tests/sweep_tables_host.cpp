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
FRAME_STUB(x264hip_launch_slice_plain) FRAME_STUB(x264hip_launch_slice_rd) FRAME_STUB(x264hip_launch_slice_rf) FRAME_STUB(x264hip_launch_slice_ll)
FRAME_STUB(x264hip_launch_slice_ll_rf) FRAME_STUB(x264hip_launch_slice_b) FRAME_STUB(x264hip_launch_slice_bt)
FRAME_STUB(x264hip_launch_psy_rd) FRAME_STUB(x264hip_launch_psy_rf) FRAME_STUB(x264hip_launch_psy_bt)
CHAINS_STUB(x264hip_launch_slice_rd_ch) CHAINS_STUB(x264hip_launch_slice_rf_ch) CHAINS_STUB(x264hip_launch_slice_ll_ch)
CHAINS_STUB(x264hip_launch_slice_ll_rf_ch) CHAINS_STUB(x264hip_launch_slice_bt_ch)
CHAINS_STUB(x264hip_launch_psy_rd_ch) CHAINS_STUB(x264hip_launch_psy_rf_ch) CHAINS_STUB(x264hip_launch_psy_bt_ch)

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

// ---- which kind codes a sweep: the `if` chain at the end of sweep_build, and the forwarding rule its launch functions then applied --
// psy-trellis on a launch of a lossy raster kernel went to the psy-trellis kernel of the same shape, both B kinds to the one extended kernel
static void check_sweep_kind()
{
    int checked = 0;
    for (int code = 0; code < 2 * 2 * 2 * 3 * 2 * 2; code++) {
        int c = code;
        const bool has_rd = c % 2; c /= 2;
        const bool is_b = c % 2; c /= 2;
        const bool lossless = c % 2; c /= 2;
        const int mbrd = c % 3; c /= 3;
        const bool psy = c % 2; c /= 2;
        const bool extended_b = c % 2;
        // skipped, because sweep_build refuses them before it selects: a B slice without the raster variant's parameters or with lossless
        // on ("a B slice needs ... .rd", "lossless B slices are not built"); psy-trellis with lossless ("lossless with psy-trellis"); and
        // psy-trellis without the raster variant's parameters, which is where the setting lives (x264hip_slice_rd.psy_trellis)
        if ((is_b && (!has_rd || lossless)) || (psy && (lossless || !has_rd))) continue;
        int want = SW_KIND_PLAIN;
        if (has_rd) {
            if (is_b) want = extended_b ? SW_KIND_BT : SW_KIND_B;
            else if (lossless) want = mbrd >= 2 ? SW_KIND_LL_RF : SW_KIND_LL;
            else want = mbrd >= 2 ? SW_KIND_RF : SW_KIND_RD;
        }
        if (psy) {
            if (want == SW_KIND_RD) want = SW_KIND_PSY_RD;
            else if (want == SW_KIND_RF) want = SW_KIND_PSY_RF;
            else if (want == SW_KIND_B || want == SW_KIND_BT) want = SW_KIND_PSY_BT;
        }
        const int got = sweep_kind(has_rd, is_b, lossless, mbrd, psy, extended_b);
        CHECK(got == want, "sweep_kind(rd %d, b %d, lossless %d, mbrd %d, psy %d, extended %d) = %d, not %d", has_rd, is_b, lossless, mbrd, psy, extended_b, got, want);
        checked++;
    }
    CHECK(checked == 12 + 12 + 6 + 12, "%d combinations checked", checked);       // no rd; B; lossless I / P; lossy I / P with psy-trellis and without
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
    // a table is all-lossless or not at all, all-psy-trellis or not at all: refused before anything is placed, the lossless count first
    const int n_ll = cnt[SW_KIND_LL] + cnt[SW_KIND_LL_RF], n_psy = cnt[SW_KIND_PSY_RD] + cnt[SW_KIND_PSY_RF] + cnt[SW_KIND_PSY_BT];
    const int want_mixed = n_ll && n_ll != n ? SW_LOSSLESS : n_psy && n_psy != n ? SW_PSY : SW_LOSSY;
    int n_mixed = -1;
    const int mixed = sweep_mixed_family(cnt, &n_mixed);
    CHECK(mixed == want_mixed, "family %d reported as mixed, not %d", mixed, want_mixed);
    if (want_mixed != SW_LOSSY) {
        const int want_n = want_mixed == SW_LOSSLESS ? n_ll : n_psy;
        CHECK(n_mixed == want_n, "%d entries of the mixed family %d reported, not %d", n_mixed, mixed, want_n);
        return;
    }
    // the B kernel's stream: its own beside an I / P kernel, or where nothing joins it to the context's
    const int n_b = cnt[SW_KIND_BT] + cnt[SW_KIND_PSY_BT], n_ip = cnt[SW_KIND_RD] + cnt[SW_KIND_RF] + cnt[SW_KIND_PSY_RD] + cnt[SW_KIND_PSY_RF];
    for (int join = 0; join < 2; join++)
        CHECK(sweep_two_streams(cnt, join != 0) == (n_b && (n_ip || !join)), "%d B and %d I / P entries, join %d: two streams %d", n_b, n_ip, join, (int)sweep_two_streams(cnt, join != 0));
    // the walk
    int base[SW_N_KINDS], at[SW_N_KINDS];
    sweep_place(cnt, base);
    memcpy(at, base, sizeof(at));
    for (int i = 0; i < n; i++) { CHECK(at[kinds[i]] < n, "placement past the table"); if (at[kinds[i]] < n) got[at[kinds[i]]++] = tmp[i]; }
    // what it replaced: [RD | RF | BT], [LL | LL_RF], and the psy-trellis kernels where the lossy ones of the same shape stood
    int wbase[SW_N_KINDS] = {0}, wat[SW_N_KINDS];
    wbase[SW_KIND_RD] = 0; wbase[SW_KIND_RF] = cnt[SW_KIND_RD]; wbase[SW_KIND_BT] = wbase[SW_KIND_RF] + cnt[SW_KIND_RF];
    wbase[SW_KIND_LL] = 0; wbase[SW_KIND_LL_RF] = cnt[SW_KIND_LL];
    wbase[SW_KIND_PSY_RD] = 0; wbase[SW_KIND_PSY_RF] = cnt[SW_KIND_PSY_RD]; wbase[SW_KIND_PSY_BT] = wbase[SW_KIND_PSY_RF] + cnt[SW_KIND_PSY_RF];
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
    if (cnt[SW_KIND_PSY_RD]) w.push_back({"x264hip_launch_psy_rd_ch", wbase[SW_KIND_PSY_RD], cnt[SW_KIND_PSY_RD], s});
    if (cnt[SW_KIND_PSY_RF]) w.push_back({"x264hip_launch_psy_rf_ch", wbase[SW_KIND_PSY_RF], cnt[SW_KIND_PSY_RF], s});
    if (cnt[SW_KIND_PSY_BT]) w.push_back({"x264hip_launch_psy_bt_ch", wbase[SW_KIND_PSY_BT], cnt[SW_KIND_PSY_BT], sb});
    CHECK(launched.size() == w.size(), "%zu launches, not %zu", launched.size(), w.size());
    for (size_t i = 0; i < launched.size() && i < w.size(); i++)
        CHECK(launched[i].fn == w[i].fn && launched[i].at == w[i].at && launched[i].n == w[i].n && launched[i].stream == w[i].stream,
              "launch %zu: %s at %ld, %d entries; expected %s at %ld, %d entries (or the other stream)", i, launched[i].fn.c_str(), launched[i].at, launched[i].n,
              w[i].fn.c_str(), w[i].at, w[i].n);
}

int main()
{
    check_state_arrays();
    // the lock-step launch of every kind: the `switch` it replaced, the wavefront schedule's own launch and the psy-trellis kernels' included
    const char *frame_fn[SW_N_KINDS] = {nullptr};
    frame_fn[SW_KIND_PLAIN] = "x264hip_launch_slice_plain";
    frame_fn[SW_KIND_RD] = "x264hip_launch_slice_rd"; frame_fn[SW_KIND_RF] = "x264hip_launch_slice_rf"; frame_fn[SW_KIND_LL] = "x264hip_launch_slice_ll";
    frame_fn[SW_KIND_LL_RF] = "x264hip_launch_slice_ll_rf"; frame_fn[SW_KIND_B] = "x264hip_launch_slice_b"; frame_fn[SW_KIND_BT] = "x264hip_launch_slice_bt";
    frame_fn[SW_KIND_PSY_RD] = "x264hip_launch_psy_rd"; frame_fn[SW_KIND_PSY_RF] = "x264hip_launch_psy_rf"; frame_fn[SW_KIND_PSY_BT] = "x264hip_launch_psy_bt";
    for (int k = 0; k < SW_N_KINDS; k++) {
        CHECK(k_sweep_kinds[k].frame != nullptr && frame_fn[k] != nullptr, "kind %d: no lock-step launch", k);
        if (!k_sweep_kinds[k].frame || !frame_fn[k]) continue;
        launched.clear();
        k_sweep_kinds[k].frame(SwArgs(), SwRefs(), SwRd(), nullptr);
        CHECK(launched.size() == 1 && launched[0].fn == frame_fn[k], "kind %d launches %s", k, launched.empty() ? "nothing" : launched[0].fn.c_str());
    }
    check_sweep_kind();
    // every mix of 0..2 entries of every kind a chain table can hold (PLAIN is refused: the table belongs to the raster variant), with
    // a stream of its own for the B kernel and without
    int cnt[SW_N_KINDS], mixes = 0;
    for (int code = 0; code < 19683; code++) {
        cnt[SW_KIND_PLAIN] = 0;
        for (int k = 1, c = code; k < SW_N_KINDS; k++, c /= 3) cnt[k] = c % 3;
        for (int two = 0; two < 2; two++) check_kinds(cnt, two != 0);
        mixes++;
    }
    printf("%d mixes, %d failures\n", mixes, failures);
    return failures != 0;
}
