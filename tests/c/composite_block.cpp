// The automatic block length of mhw_composite() (xmhw_amd/csrc/stage_blocks.h, composite_auto_block) for the (T, C, D)
// triples given on the command line, as a JSON list of [T, C, D, block]: tests/test_host_composite_block.py pins them.
// The header is plain C++ and needs no device.
#include <cstdio>
#include <cstdlib>

#include "../../xmhw_amd/csrc/stage_blocks.h"

int main(int argc, char** argv) {
    std::printf("[");
    for (int i = 1; i + 2 < argc; i += 3) {
        const long long T = std::atoll(argv[i]), C = std::atoll(argv[i + 1]), D = std::atoll(argv[i + 2]);
        std::printf("%s[%lld, %lld, %lld, %lld]", i > 1 ? ", " : "", T, C, D,
                    static_cast<long long>(xmhw::composite_auto_block(T, C, D)));
    }
    std::printf("]\n");
    return 0;
}
