// pcio::read_ply_mesh (cloud_map_evaluation_amd/host/pcd_io.hpp) on the files named on the command line, under the host sanitizers
// (built by tests/test_ply_mesh_cpu.py with -fsanitize=address,undefined): every file is read; "ok <vertices> <triangles>" or
// "fail <message>" per file.  A reader that runs past a buffer on a malformed file ends the program instead.
#include <cstdio>

#include "../../cloud_map_evaluation_amd/host/pcd_io.hpp"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<double> xyz;
        std::vector<int32_t> tri;
        std::string err;
        if (pcio::read_ply_mesh(argv[i], xyz, tri, &err)) {
            for (const int32_t t : tri)  // every index the reader let through addresses a vertex
                if (t < 0 || (size_t) t >= xyz.size() / 3) return 2;
            std::printf("ok %zu %zu\n", xyz.size() / 3, tri.size() / 3);
        } else {
            std::printf("fail %s\n", err.c_str());
        }
    }
    return 0;
}
