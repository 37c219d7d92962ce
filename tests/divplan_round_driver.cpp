// wafer_divplan_q_round (the host statement of the fp64 division an UNCHECKED divisor runs: q, then one remainder round) over a file
// of doubles: tests/test_full_forms_host.py builds and runs this to hold the path the full-form kernels take to x / den.
//   divplan_round_driver <in: raw float64 operands> <out: raw float64 quotients> <den> <zh> <zl>, each as 16 hex digits
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../wafer_amd/csrc/wafer_divplan.h"

static double from_bits(const char *hex)
{
    const uint64_t u = (uint64_t)std::strtoull(hex, nullptr, 16);
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    std::vector<double> x((size_t)bytes / sizeof(double));
    if (std::fread(x.data(), sizeof(double), x.size(), in) != x.size()) return 4;
    std::fclose(in);
    const double den = from_bits(argv[3]), zh = from_bits(argv[4]), zl = from_bits(argv[5]);
    for (double &v : x) v = wafer_divplan_q_round(v, den, zh, zl);
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 5;
    if (std::fwrite(x.data(), sizeof(double), x.size(), out) != x.size()) return 6;
    return std::fclose(out) == 0 ? 0 : 7;
}
