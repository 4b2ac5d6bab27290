// The automatic block lengths of the stage kernels (xmhw_amd/csrc/stage_blocks.h) over a fixed sweep, as JSON: extents
// around the 64-step word, the 256-step least block and the 4096-step cap, cell counts around one workgroup and around
// the 2048 workgroups that fill the chip.  tests/test_host_stage_blocks.py compares the output with
// tests/golden/stage_blocks.json.
#include <stdio.h>

#include "../../xmhw_amd/csrc/stage_blocks.h"

using namespace xmhw;

static const int64_t kExtents[] = {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 14610, 100000};
static const int64_t kCells[] = {1, 255, 256, 257, 65536, 524287, 524288, 1036800};
static const int32_t kWindows[] = {1, 16, 84, 255};
static const int32_t kLags[] = {1, 8, 9, 64};
static const int64_t kGrids[][2] = {{1, 1}, {180, 360}, {720, 1440}};
static const int kLagGroup = 8;                      // kCooccurLagGroup (kernels.h): the lags of one grid.z slice

static const char* sep = "";
static void row(long long a, long long b, long long c, long long r, bool three = true) {
    if (three) printf("%s[%lld, %lld, %lld, %lld]", sep, a, b, c, r);
    else printf("%s[%lld, %lld, %lld]", sep, a, b, r);
    sep = ", ";
}
static void field(const char* head) {
    printf("%s", head);
    sep = "";
}

int main() {
    field("{\"class_days\": [");
    for (int64_t t : kExtents)
        for (int64_t c : kCells) row(t, c, 0, class_days_auto_block(t, c), false);
    field("],\n \"heat_stress\": [");
    for (int64_t t : kExtents)
        for (int64_t c : kCells)
            for (int32_t w : kWindows) row(t, c, w, heat_stress_auto_block(t, c, w));
    field("],\n \"displacement\": [");
    for (int64_t t : kExtents)
        for (auto& g : kGrids) row(t, g[0], g[1], displacement_auto_block(t, g[0], g[1]));
    field("],\n \"cooccur\": [");
    for (int64_t w : kExtents)
        for (int64_t c : kCells)
            for (int32_t l : kLags) row(w, c, l, cooccur_auto_block(w, c, (l + kLagGroup - 1) / kLagGroup));
    printf("]}\n");
    return 0;
}
