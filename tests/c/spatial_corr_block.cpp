// The automatic block length and the offset groups of spatial_correlation() (xmhw_amd/csrc/stage_blocks.h,
// spatial_corr_auto_block, spatial_corr_group, spatial_corr_groups) for the (nt, ny, nx, rows, D) tuples given on the
// command line, as a JSON list of [nt, ny, nx, rows, D, group, groups, block]: tests/test_host_spatial_corr_block.py pins
// them.  The header is plain C++ and needs no device.
#include <cstdio>
#include <cstdlib>

#include "../../xmhw_amd/csrc/stage_blocks.h"

int main(int argc, char** argv) {
    std::printf("[");
    for (int i = 1; i + 4 < argc; i += 5) {
        const long long nt = std::atoll(argv[i]), ny = std::atoll(argv[i + 1]), nx = std::atoll(argv[i + 2]),
                        rows = std::atoll(argv[i + 3]), D = std::atoll(argv[i + 4]);
        std::printf("%s[%lld, %lld, %lld, %lld, %lld, %lld, %lld, %lld]", i > 1 ? ", " : "", nt, ny, nx, rows, D,
                    static_cast<long long>(xmhw::spatial_corr_group(D)), static_cast<long long>(xmhw::spatial_corr_groups(D)),
                    static_cast<long long>(xmhw::spatial_corr_auto_block(nt, ny, nx, rows, D)));
    }
    std::printf("]\n");
    return 0;
}
