// tum_io.hpp — the positions of a TUM-format trajectory (text lines `t x y z qx qy qz qw`; `#` comments and blank lines are skipped).
// Header-only, no dependencies.  Only the positions are kept (evaluate_observable casts from them); all eight fields of a line must
// still be finite numbers and nothing may follow them: a malformed line is refused with its line number.
#pragma once

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

namespace tumio {

// xyz: [n][3] positions in file order.  false + *err on a file that cannot be read, holds a malformed line, or holds no pose.
inline bool read_tum_positions(const std::string &path, std::vector<double> &xyz, std::string *err = nullptr) {
    auto fail = [&](const std::string &m) {
        if (err) *err = m;
        xyz.clear();
        return false;
    };
    xyz.clear();
    std::ifstream in(path);
    if (!in) return fail("cannot open trajectory '" + path + "'");
    std::string line;
    long long no = 0;
    while (std::getline(in, line)) {
        ++no;
        size_t b = line.find_first_not_of(" \t\r");
        if (b == std::string::npos || line[b] == '#') continue;
        const char *p = line.c_str() + b;
        double f[8];
        for (int k = 0; k < 8; ++k) {
            char *end = nullptr;
            f[k] = std::strtod(p, &end);
            if (end == p || !std::isfinite(f[k]))
                return fail("trajectory '" + path + "' line " + std::to_string(no) + ": expected 8 finite numbers `t x y z qx qy qz qw`, field " +
                            std::to_string(k + 1) + " is missing or not a number");
            p = end;
            if (k < 7 && *p != ' ' && *p != '\t')
                return fail("trajectory '" + path + "' line " + std::to_string(no) + ": expected 8 finite numbers `t x y z qx qy qz qw`, field " +
                            std::to_string(k + 2) + " is missing or not a number");
        }
        while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
        if (*p != '\0') return fail("trajectory '" + path + "' line " + std::to_string(no) + ": text after the eighth field");
        xyz.push_back(f[1]);
        xyz.push_back(f[2]);
        xyz.push_back(f[3]);
    }
    if (in.bad()) return fail("reading trajectory '" + path + "' failed");
    if (xyz.empty()) return fail("trajectory '" + path + "' holds no pose");
    return true;
}

}  // namespace tumio
