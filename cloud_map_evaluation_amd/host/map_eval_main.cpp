// map_eval_main.cpp — entry point mirroring map_eval/src/map_eval_main.cpp:211-244: reads ../config/config.yaml by default
// (the reference hard-codes that path and has the argv override commented out; here argv[1] works), prints the banner
// essentials, runs MapEval::process().  Extra modes used by the tests (no GPU needed):
//   map_eval --parse-config <yaml>   print the parsed Param as JSON (an infinite mesh_max_distance as the token Infinity, which
//                                    Python's json reads; strict JSON has no infinity)
//   map_eval --cloud-info <pcd|ply>  print point count and coordinate sums after NaN/inf removal
//   map_eval --mesh-info <ply>       print the mesh's counts, area and bounding box from the reader alone
//
// Multi-GPU (`num_gpus: N` in the YAML; not a reference key): the process forks N - 1 children BEFORE anything touches HIP;
// rank r drives device gpu_device + r (one process per GPU), the ranks meet in an RCCL communicator whose ncclUniqueId rank 0
// publishes in a file next to the results (host/dist_comm.hpp), rank 0 writes every result file.  Test hooks:
// MAPEVAL_FORCE_DIST=1 takes the distributed path with ONE rank (every collective goes through RCCL);
// MAPEVAL_COMM=file + MAPEVAL_SINGLE_DEVICE=1 run N ranks on one GPU with file-based collectives (RCCL refuses two ranks on a
// device).
#include <sys/wait.h>
#include <signal.h>
#include <sys/prctl.h>
#include <unistd.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iomanip>
#include <iostream>
#include <thread>

#include "dist_comm.hpp"
#include "map_eval.h"
#include "pcd_io.hpp"

namespace {
std::vector<pid_t> g_children;  // launcher only
// SIGCHLD in the launcher: a child that ended badly ends the job (async-signal-safe calls only)
void on_child_exit(int) {
    int st = 0;
    pid_t pid;
    while ((pid = waitpid(-1, &st, WNOHANG)) > 0) {
        const bool bad = !(WIFEXITED(st) && WEXITSTATUS(st) == 0);
        for (pid_t &c : g_children)
            if (c == pid) c = -1;  // reaped
        if (bad) {
            for (pid_t c : g_children)
                if (c > 0) kill(c, SIGKILL);
            static const char msg[] = "\n[ERROR] a rank of the multi-GPU run failed: stopping the others\n";
            (void) !write(2, msg, sizeof msg - 1);
            _exit(EXIT_FAILURE);
        }
    }
}
}  // namespace

int main(int argc, char **argv) {
    // HIP runtime setting, before its first call: kernel arguments in device memory (a step is several hundred launches; 0.2-0.3 ms
    // per step on the bench scene).  An explicit HIP_FORCE_DEV_KERNARG in the environment wins.
    setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
    std::string config_file = "../config/config.yaml";
    if (argc > 2 && std::string(argv[1]) == "--parse-config") {
        try {
            std::cout << paramToJson(loadParametersFromYAML(argv[2])) << std::endl;
            return EXIT_SUCCESS;
        } catch (const std::exception &e) {
            std::cerr << "\n[ERROR] Failed to load configuration: " << e.what() << "\n";
            return EXIT_FAILURE;
        }
    }
    if (argc > 2 && std::string(argv[1]) == "--cloud-info") {
        std::vector<double> xyz, nrm;
        std::string err, path = argv[2];
        const bool ok = path.size() > 4 && path.substr(path.size() - 4) == ".ply" ? pcio::read_ply(path, xyz, &err, &nrm)
                                                                                     : pcio::read_pcd(path, xyz, &err, &nrm);
        if (!ok) {
            std::cerr << "ERROR: " << err << std::endl;
            return EXIT_FAILURE;
        }
        double s[3] = {0, 0, 0}, sn[3] = {0, 0, 0};
        for (size_t i = 0; i < xyz.size() / 3; ++i)
            for (int d = 0; d < 3; ++d) s[d] += xyz[3 * i + d];
        for (size_t i = 0; i < nrm.size() / 3; ++i)
            for (int d = 0; d < 3; ++d) sn[d] += nrm[3 * i + d];
        std::cout << std::setprecision(17) << "{\"points\": " << xyz.size() / 3 << ", \"sum\": [" << s[0] << ", " << s[1] << ", " << s[2]
                  << "], \"normals\": " << nrm.size() / 3 << ", \"normal_sum\": [" << sn[0] << ", " << sn[1] << ", " << sn[2] << "]}"
                  << std::endl;
        return EXIT_SUCCESS;
    }
    if (argc > 2 && std::string(argv[1]) == "--mesh-info") {
        std::vector<double> xyz;
        std::vector<int32_t> tri;
        std::string err;
        if (!pcio::read_ply_mesh(argv[2], xyz, tri, &err)) {
            std::cerr << "ERROR: " << err << std::endl;
            return EXIT_FAILURE;
        }
        // area and the degenerate test as me_mesh_upload forms them; the box over the referenced vertices
        double area = 0.0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        size_t n_deg = 0;
        for (size_t t = 0; t < tri.size() / 3; ++t) {
            const double *a = &xyz[3 * (size_t) tri[3 * t]], *b = &xyz[3 * (size_t) tri[3 * t + 1]], *c = &xyz[3 * (size_t) tri[3 * t + 2]];
            const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
            n_deg += nx == 0.0 && ny == 0.0 && nz == 0.0;
            area += 0.5 * std::sqrt((nx * nx + ny * ny) + nz * nz);
            for (const double *p : {a, b, c})
                for (int d = 0; d < 3; ++d) lo[d] = std::fmin(lo[d], p[d]), hi[d] = std::fmax(hi[d], p[d]);
        }
        if (tri.empty())
            for (int d = 0; d < 3; ++d) lo[d] = hi[d] = 0.0;
        std::cout << std::setprecision(17) << "{\"vertices\": " << xyz.size() / 3 << ", \"triangles\": " << tri.size() / 3
                  << ", \"degenerate\": " << n_deg << ", \"area\": " << area << ", \"bbox\": [" << lo[0] << ", " << lo[1] << ", " << lo[2]
                  << ", " << hi[0] << ", " << hi[1] << ", " << hi[2] << "]}" << std::endl;
        return EXIT_SUCCESS;
    }
    if (argc > 1) config_file = argv[1];
    // `map_eval config.yaml --repeat N` (measurement aid, single GPU): the evaluation N times in this process — the first run pays the
    // cold start (runtime and code-object load, every device allocation, the GPU's clocks coming up from idle after the file reads),
    // the later ones show what the same call costs a long-lived caller (profiles/host_one_call.py)
    int repeat = 1;
    if (argc > 3 && std::string(argv[2]) == "--repeat") repeat = std::max(1, std::atoi(argv[3]));

    std::cout << "Loading configuration from: " << config_file << "\n";
    Param param;
    try {
        param = loadParametersFromYAML(config_file);
    } catch (const std::exception &e) {
        std::cerr << "\n[ERROR] Failed to load configuration: " << e.what() << "\n";
        return EXIT_FAILURE;  // map_eval_main.cpp:224-227
    }
    std::cout << "MapEval (MI355X / HIP engine): A Unified Framework for Map Evaluation\n"
              << "CPU Cores: " << std::thread::hardware_concurrency() << "\n";
    // ---- multi-GPU launcher: one process per GPU ----
    const bool forced = std::getenv("MAPEVAL_FORCE_DIST") && std::string(std::getenv("MAPEVAL_FORCE_DIST")) == "1";
    const int world = param.num_gpus;
    int rank = 0;
    std::vector<pid_t> children;
    const long launcher_pid = (long) getpid();
    if (world > 1) {
        std::cout.flush();
        // The SIGCHLD handler is installed BEFORE the first fork, blocked until the children are recorded: a child
        // that dies early is not missed, and SA_RESTART keeps rank 0's blocking system calls (file I/O, the file transport's polling)
        // from failing with EINTR when ranks exit.
        struct sigaction sa;
        std::memset(&sa, 0, sizeof sa);
        sa.sa_handler = on_child_exit;
        sa.sa_flags = SA_NOCLDSTOP | SA_RESTART;
        sigset_t chld, old_mask;
        sigemptyset(&chld);
        sigaddset(&chld, SIGCHLD);
        sigprocmask(SIG_BLOCK, &chld, &old_mask);
        sigaction(SIGCHLD, &sa, nullptr);
        for (int r = 1; r < world; ++r) {
            const pid_t pid = fork();
            if (pid < 0) {
                std::cerr << "[ERROR] fork failed" << std::endl;
                for (pid_t c : children) kill(c, SIGKILL);
                return EXIT_FAILURE;
            }
            if (pid == 0) {
                rank = r;
                children.clear();
                signal(SIGCHLD, SIG_DFL);
                sigprocmask(SIG_SETMASK, &old_mask, nullptr);
                // a rank never outlives the launcher (rank 0): no orphan is left spinning in a collective
                prctl(PR_SET_PDEATHSIG, SIGKILL);
                if (getppid() != (pid_t) launcher_pid) _exit(EXIT_FAILURE);
                break;
            }
            children.push_back(pid);
        }
        if (rank == 0) {
            // ... and the launcher does not outlive a failed rank: RCCL collectives have no timeout, so a rank that exits with an
            // error (GPU fault, out of memory, a failed library call) takes the whole job down instead of hanging it
            g_children = children;
            sigprocmask(SIG_SETMASK, &old_mask, nullptr);  // pending SIGCHLDs (children that have died already) are delivered now
        }
    }
    const bool single_device = std::getenv("MAPEVAL_SINGLE_DEVICE") && std::string(std::getenv("MAPEVAL_SINGLE_DEVICE")) == "1";
    param.dist_rank = rank;
    if (!single_device) param.gpu_device += rank;
    std::unique_ptr<medist::Comm> comm;
    if (world > 1 || forced) {
        std::error_code ec;
        std::filesystem::create_directories(param.evaluation_map_pcd_path_ + "map_results", ec);
        const std::string base = param.evaluation_map_pcd_path_ + "map_results/.mapeval_comm_" + std::to_string(launcher_pid);
        if (std::getenv("MAPEVAL_COMM") && std::string(std::getenv("MAPEVAL_COMM")) == "file") {
            std::filesystem::create_directories(base, ec);
            auto c = std::make_unique<medist::FileComm>();
            c->init(rank, world, base);
            comm = std::move(c);
        } else {
            auto c = std::make_unique<medist::RcclComm>();
            if (!c->init(rank, world, param.gpu_device, base + ".id")) {
                std::cerr << "[ERROR] rank " << rank << ": RCCL bootstrap failed: " << c->err << std::endl;
                if (rank > 0) _exit(EXIT_FAILURE);
                signal(SIGCHLD, SIG_DFL);
                for (pid_t pid : children) {  // they fail on the same pre-flight; only then are the bootstrap files removed
                    int st = 0;
                    (void) waitpid(pid, &st, 0);
                }
                medist::RcclComm::remove_bootstrap_files(base + ".id", world);
                return EXIT_FAILURE;
            }
            comm = std::move(c);
        }
    }
    if (rank == 0) param.printParam();
    std::cout << "Starting evaluation...\n"
              << "================================================================================\n\n";
    int rc = 0;
    for (int it = 0; it < (world > 1 ? 1 : repeat) && rc == 0; ++it) {
        MapEval map_eval(param);
        if (comm) map_eval.setComm(comm.get(), forced);
        rc = map_eval.process();
    }
    if (rc != 0 && world > 1) {
        // a failed rank leaves at once (no communicator tear-down: its peers may be inside a collective it will never join)
        if (rank > 0) _exit(EXIT_FAILURE);
        signal(SIGCHLD, SIG_DFL);
        for (pid_t c : g_children)
            if (c > 0) kill(c, SIGKILL);
        std::cerr << "[ERROR] rank 0 failed: the other ranks were stopped" << std::endl;
        _exit(EXIT_FAILURE);
    }
    comm.reset();
    if (rank > 0) _exit(rc == 0 ? EXIT_SUCCESS : EXIT_FAILURE);
    if (world > 1) {  // the children still running are reaped here; the SIGCHLD handler has taken the others (and checked them)
        signal(SIGCHLD, SIG_DFL);
        for (pid_t pid : g_children) {
            if (pid <= 0) continue;
            int st = 0;
            if (waitpid(pid, &st, 0) > 0 && !(WIFEXITED(st) && WEXITSTATUS(st) == 0)) rc = rc ? rc : -1;
        }
    }
    if (world > 1 && std::getenv("MAPEVAL_COMM") && std::string(std::getenv("MAPEVAL_COMM")) == "file") {
        std::error_code ec;
        std::filesystem::remove_all(param.evaluation_map_pcd_path_ + "map_results/.mapeval_comm_" + std::to_string(launcher_pid), ec);
    }
    std::cout << "\n================================================================================\n"
              << (rc == 0 ? "Evaluation completed successfully!\n" : "Evaluation FAILED.\n")
              << "================================================================================\n\n";
    return rc == 0 ? EXIT_SUCCESS : EXIT_FAILURE;  // the reference ignores process()'s return value (:237)
}
