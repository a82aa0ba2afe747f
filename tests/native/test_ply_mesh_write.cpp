// pcio::write_ply_mesh -> pcio::read_ply_mesh (cloud_map_evaluation_amd/host/pcd_io.hpp) under the host sanitizers (built by
// tests/test_ply_mesh_write_cpu.py with -fsanitize=address,undefined): meshes written into the directory named on the command line
// come back bit for bit, a zero-triangle mesh and an empty one included; a bad index is refused.  Prints "ok" and returns 0.
#include <cstdio>
#include <cstring>

#include "../../cloud_map_evaluation_amd/host/pcd_io.hpp"

static int round_trip(const std::string &path, const std::vector<double> &xyz, const std::vector<int32_t> &tri) {
    std::string err;
    if (!pcio::write_ply_mesh(path, xyz, tri, &err)) {
        std::printf("write failed: %s\n", err.c_str());
        return 1;
    }
    std::vector<double> x2{1.0};
    std::vector<int32_t> t2{5};
    if (!pcio::read_ply_mesh(path, x2, t2, &err)) {
        std::printf("read failed: %s\n", err.c_str());
        return 1;
    }
    if (x2.size() != xyz.size() || t2.size() != tri.size()) return 2;
    if (!xyz.empty() && std::memcmp(x2.data(), xyz.data(), xyz.size() * 8) != 0) return 3;  // bit for bit: -0.0, denormals, huge values
    if (!tri.empty() && std::memcmp(t2.data(), tri.data(), tri.size() * 4) != 0) return 4;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 64;
    const std::string dir = argv[1];
    std::vector<double> xyz = {0.0, -0.0, 1.0, 4.0e5 + 0.1, -3.0e5 - 0.3, 50.25, 4.9406564584124654e-324, 1.7976931348623157e308, -1e-300,
                               0.1, 0.2, 0.30000000000000004, 1.0 / 3.0, 2.0 / 3.0, 5.0};
    std::vector<int32_t> tri = {0, 1, 2, 2, 3, 4, 4, 4, 0, 3, 1, 0};
    int rc = round_trip(dir + "/mesh.ply", xyz, tri);
    if (rc) return rc;
    rc = round_trip(dir + "/no_faces.ply", xyz, {});  // a zero-triangle mesh
    if (rc) return 10 + rc;
    rc = round_trip(dir + "/empty.ply", {}, {});
    if (rc) return 20 + rc;
    std::vector<double> big;
    std::vector<int32_t> bt;
    for (int i = 0; i < 3000; ++i) big.push_back(i * 0.37 - 500.0);
    for (int i = 0; i + 2 < 1000; ++i) bt.insert(bt.end(), {i, i + 1, i + 2});
    rc = round_trip(dir + "/strip.ply", big, bt);
    if (rc) return 30 + rc;
    std::string err;
    if (pcio::write_ply_mesh(dir + "/bad.ply", xyz, {0, 1, 5}, &err) || err.find("outside") == std::string::npos) return 40;
    if (pcio::write_ply_mesh(dir + "/bad.ply", xyz, {0, -1, 2}, &err)) return 41;
    if (pcio::write_ply_mesh(dir + "/bad.ply", xyz, {0, 1}, &err)) return 42;
    if (pcio::write_ply_mesh(dir + "/no/such/dir/m.ply", xyz, tri, &err) || err.find("cannot open") == std::string::npos) return 43;
    std::printf("ok\n");
    return 0;
}
