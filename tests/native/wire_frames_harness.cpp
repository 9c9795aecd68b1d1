// Host-only harness for the frame-wise wire parse (pekf_wire_parse_frames, csrc/pekf_wire.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_wire_repair_cpu.py builds and runs it; no GPU, no
// HIP).  Each argument is a file of whole 100-byte frames: they are parsed from an exactly-sized heap copy into
// exactly-sized outputs, so a read or write past either end is a sanitizer report, and the statuses are printed
// as one digit per frame.  Then frames of random bytes, NULs and '#' starts included, go the same way.
// pekf::set_error (pekf_capi.hip in the library) is replaced by a printing stub.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pekf.h"

namespace pekf {
int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char msg[512];
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    fprintf(stderr, "error %d: %s\n", code, msg);
    return code;
}
}  // namespace pekf

// parses the frames of an exactly-sized copy; prints "<label> rc=<status> n=<frames> st=<digits> t=<sum> v=<sum>"
static int run(const char *label, const std::vector<uint8_t> &bytes) {
    const int64_t n = (int64_t)(bytes.size() / PEKF_WIRE_FRAME_BYTES);
    std::vector<uint8_t> exact(bytes.begin(), bytes.begin() + n * PEKF_WIRE_FRAME_BYTES);
    std::vector<uint8_t> st(n), ph(n), ty(n);
    std::vector<double> xyz(3 * n);
    std::vector<int64_t> t(n);
    const int rc = pekf_wire_parse_frames(n, exact.data(), st.data(), ph.data(), ty.data(), xyz.data(), t.data());
    std::string digits;
    uint64_t tsum = 0;
    double vsum = 0;
    for (int64_t f = 0; f < n; ++f) {
        digits += (char)('0' + st[f]);
        if (st[f] != PEKF_WIRE_MESSAGE && (ph[f] || ty[f] || t[f] || xyz[3 * f] != 0 || xyz[3 * f + 1] != 0 ||
                                          xyz[3 * f + 2] != 0))
            return 1;  // anything but a processed frame leaves zeros
        tsum += (uint64_t)t[f];
        for (int k = 0; k < 3; ++k) vsum += std::isfinite(xyz[3 * f + k]) ? xyz[3 * f + k] : 0.0;
    }
    printf("%s rc=%d n=%lld st=%s t=%llu v=%.17g\n", label, rc, (long long)n, digits.c_str(),
           (unsigned long long)tsum, vsum);
    return 0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<uint8_t> bytes;
        if (std::FILE *f = std::fopen(argv[i], "rb")) {
            uint8_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
            std::fclose(f);
        }
        if (run(argv[i], bytes)) return 2;
    }
    // random frames: every byte value; every fourth starts as a message does; some are cut by NULs, some have none
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    std::vector<uint8_t> noise(4000 * PEKF_WIRE_FRAME_BYTES);
    for (size_t f = 0; f < noise.size() / PEKF_WIRE_FRAME_BYTES; ++f) {
        uint8_t *fr = noise.data() + f * PEKF_WIRE_FRAME_BYTES;
        const bool text = f % 3 == 1;  // bytes of the message alphabet: far more of them parse some way
        for (int j = 0; j < PEKF_WIRE_FRAME_BYTES; ++j)
            fr[j] = text ? (uint8_t)"0123456789.,:-+eEtx# \0"[next() % 22] : (uint8_t)(next() >> 56);
        if (f % 4 == 0) std::memcpy(fr, "#3,1:", 5);
        if (f % 8 == 0) std::memcpy(fr + 5, "1.5,-2.25,3e2,t:", 16);
        if (f % 5 == 0)
            for (int j = 0; j < PEKF_WIRE_FRAME_BYTES; ++j) fr[j] = fr[j] ? fr[j] : (uint8_t)' ';  // no NUL at all
    }
    if (run("noise", noise)) return 2;
    if (run("empty", {})) return 2;
    const int null_rc = pekf_wire_parse_frames(1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int neg_rc = pekf_wire_parse_frames(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    printf("null rc=%d negative rc=%d\n", null_rc, neg_rc);
    return 0;
}
