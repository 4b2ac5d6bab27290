// The automatic block length of anomaly_distribution() (xmhw_amd/csrc/stage_blocks.h, distribution_auto_block) for the
// (T, C) pairs given on the command line, as a JSON list of [T, C, block]: tests/test_host_distribution_block.py pins them.
// The header is plain C++ and needs no device.
#include <cstdio>
#include <cstdlib>

#include "../../xmhw_amd/csrc/stage_blocks.h"

int main(int argc, char** argv) {
    std::printf("[");
    for (int i = 1; i + 1 < argc; i += 2) {
        const long long T = std::atoll(argv[i]), C = std::atoll(argv[i + 1]);
        std::printf("%s[%lld, %lld, %lld]", i > 1 ? ", " : "", T, C,
                    static_cast<long long>(xmhw::distribution_auto_block(T, C)));
    }
    std::printf("]\n");
    return 0;
}
