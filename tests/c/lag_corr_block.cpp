// The automatic block length of lag_correlation() (xmhw_amd/csrc/stage_blocks.h, lag_corr_auto_block) for the (T, C, L)
// triples given on the command line, as a JSON list of [T, C, L, block]: tests/test_host_lag_corr_block.py pins them.
// The header is plain C++ and needs no device.
#include <cstdio>
#include <cstdlib>

#include "../../xmhw_amd/csrc/stage_blocks.h"

int main(int argc, char** argv) {
    std::printf("[");
    for (int i = 1; i + 2 < argc; i += 3) {
        const long long T = std::atoll(argv[i]), C = std::atoll(argv[i + 1]), L = std::atoll(argv[i + 2]);
        std::printf("%s[%lld, %lld, %lld, %lld]", i > 1 ? ", " : "", T, C, L,
                    static_cast<long long>(xmhw::lag_corr_auto_block(T, C, L)));
    }
    std::printf("]\n");
    return 0;
}
