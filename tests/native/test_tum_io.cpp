// tumio::read_tum_positions (cloud_map_evaluation_amd/host/tum_io.hpp) on the files named on the command line, under the host sanitizers
// (built by tests/test_ray_model_cpu.py with -fsanitize=address,undefined): "ok <poses> <x y z of the last>" or "fail <message>" per file.
#include <cstdio>

#include "../../cloud_map_evaluation_amd/host/tum_io.hpp"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<double> xyz;
        std::string err;
        if (tumio::read_tum_positions(argv[i], xyz, &err)) {
            if (xyz.size() % 3 != 0 || xyz.empty()) return 2;
            const size_t n = xyz.size() / 3;
            std::printf("ok %zu %.17g %.17g %.17g\n", n, xyz[3 * n - 3], xyz[3 * n - 2], xyz[3 * n - 1]);
        } else {
            if (!xyz.empty()) return 3;  // a refused file leaves nothing behind
            std::printf("fail %s\n", err.c_str());
        }
    }
    return 0;
}
