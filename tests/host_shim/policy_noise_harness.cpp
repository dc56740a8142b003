// Compiles csrc/noise.h for the host (test infrastructure; tests/test_policy_noise_host.py).  Two commands:
//   philox c0 c1 c2 c3 k0 k1                       (hex words)  -> the four output words of Philox4x32-10, hex
//   draws seed traj sample0 nsamples k kind pairs  (decimal)    -> raw doubles on stdout: for sample = sample0 .. sample0 + nsamples - 1 and
//                                                                  j = 0 .. pairs - 1 the record (u1, u2, z0, z1) of normal_pair
#include <hip/hip_runtime.h>

#include "noise.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc == 8 && !std::strcmp(argv[1], "philox")) {
    uint32_t w[6], out[4];
    for (int i = 0; i < 6; ++i) w[i] = (uint32_t)std::strtoul(argv[2 + i], nullptr, 16);
    to::philox4x32_10(w, w + 4, out);
    std::printf("%08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
    return 0;
  }
  if (argc == 9 && !std::strcmp(argv[1], "draws")) {
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    const uint32_t traj = (uint32_t)std::strtoul(argv[3], nullptr, 10), s0 = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const uint32_t ns = (uint32_t)std::strtoul(argv[5], nullptr, 10), k = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const uint32_t kind = (uint32_t)std::strtoul(argv[7], nullptr, 10), pairs = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    std::vector<double> rec((size_t)ns * pairs * 4);
    size_t at = 0;
    for (uint32_t s = 0; s < ns; ++s)
      for (uint32_t j = 0; j < pairs; ++j, at += 4) {
        to::uniform_pair(seed, traj, s0 + s, k, kind, j, &rec[at], &rec[at + 1]);
        to::normal_pair(seed, traj, s0 + s, k, kind, j, &rec[at + 2], &rec[at + 3]);
      }
    return std::fwrite(rec.data(), sizeof(double), rec.size(), stdout) == rec.size() ? 0 : 2;
  }
  std::fprintf(stderr, "usage: %s philox c0 c1 c2 c3 k0 k1 | draws seed traj sample0 nsamples k kind pairs\n", argv[0]);
  return 1;
}
