// wafer_divplan_qf (the host statement of the f32fast kernels' planned division) over a file of floats: tests/test_fp32_reference.py
// builds and runs this to hold the numpy restatement in tests/fp32_reference.py to it.
//   divplan_qf_driver <in: raw float32 operands> <out: raw float32 quotients> <zh, as 8 hex digits> <zl, as 8 hex digits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../wafer_amd/csrc/wafer_divplan.h"

static float from_bits(const char *hex)
{
    const uint32_t u = (uint32_t)std::strtoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    std::vector<float> x((size_t)bytes / sizeof(float));
    if (std::fread(x.data(), sizeof(float), x.size(), in) != x.size()) return 4;
    std::fclose(in);
    const float zh = from_bits(argv[3]), zl = from_bits(argv[4]);
    for (float &v : x) v = wafer_divplan_qf(v, zh, zl);
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 5;
    if (std::fwrite(x.data(), sizeof(float), x.size(), out) != x.size()) return 6;
    return std::fclose(out) == 0 ? 0 : 7;
}
