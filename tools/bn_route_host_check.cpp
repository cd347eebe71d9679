// Stand-alone host check of vo_bn_route (include/vonoma.h) for a sanitizer build: it walks sizes, dtypes,
// alignments and record lengths through the plan, which makes no GPU call, and checks the invariants the
// launches rely on.  Build and run (no GPU needed):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -I include -I visual_onoma_to_wave_amd/csrc \
//     tools/bn_route_host_check.cpp visual_onoma_to_wave_amd/csrc/batchnorm.hip \
//     visual_onoma_to_wave_amd/csrc/vo_runtime.cpp -o visual_onoma_to_wave_amd/build/bn_route_host_check && \
//     visual_onoma_to_wave_amd/build/bn_route_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vonoma.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  const int Ms[] = {1, 3, 4, 8, 9, 45, 60, 85, 129, 257, 511, 1028, 3049, 8193, 131076, 1 << 24};
  const int Cs[] = {1, 8, 12, 65, 80, 512, 1024, 1028, 2048, 2056, 4096};
  const uintptr_t base = 1 << 20;
  const uintptr_t offs[] = {0, 2, 4, 8, 16, 60};
  long plans = 0;
  for (int M : Ms)
    for (int C : Cs)
      for (int xdt : {VO_F32, VO_BF16})
        for (int gdt : {-1, (int)VO_F32, (int)VO_BF16})
          for (uintptr_t ox : offs)
            for (uintptr_t og : offs) {
              if ((int64_t)M * C > (1LL << 30)) continue;
              std::vector<int32_t> rec(VO_BN_ROUTE_FIELDS, -7);  // exactly the record: one write past it is caught
              const void* x = ox ? (const void*)(base + ox) : nullptr;  // NULL in a plan call: aligned
              const void* dy = (const void*)(base + og);
              const void* out = (const void*)(base + ox);
              CHECK(vo_bn_route(M, C, xdt, gdt, x, gdt < 0 ? nullptr : dy, out, rec.data(), VO_BN_ROUTE_FIELDS) ==
                    VO_BN_ROUTE_FIELDS);
              ++plans;
              const int route = rec[0], V = rec[1], CV = rec[2], RL = rec[3], RB = rec[4], nb = rec[5], ab = rec[6],
                        CT = rec[7];
              const int Vx = xdt == VO_BF16 ? 8 : 4;
              CHECK(route >= 0 && route <= 2 && RB > 0 && nb > 0 && ab > 0 && RL > 0);
              if (route == 0) {
                CHECK(V == 0 && CV == 0 && (CT == 1 || CT == 64) && RL == 256 / CT && ab <= 4096);
                CHECK((int64_t)nb * RB >= M && (int64_t)(nb - 1) * RB < M);
              } else {
                const int rows = route == 2 ? M / V : M;
                CHECK(V == Vx && CT == 0 && CV >= 1 && CV <= 256 && RL == 256 / CV && RB % RL == 0 && nb <= 128);
                CHECK(route == 2 ? (C == 1 && M % V == 0 && CV == 1) : (C % V == 0 && CV == C / V));
                CHECK((int64_t)nb * RB >= rows && (int64_t)(nb - 1) * RB < rows);
                CHECK(((int64_t)ab * 256) % CV == 0);  // every thread of the apply grid keeps one vector column
                // the alignment rule: 16 bytes for x, the output and dy (8 for a bf16 dy beside an fp32 x)
                CHECK(ox % 16 == 0);
                if (gdt >= 0) CHECK(og % (xdt == VO_F32 && gdt == VO_BF16 ? 8 : 16) == 0);
                CHECK(!(gdt == VO_F32 && xdt == VO_BF16));
                // the workspace the entry points are given holds the partials
                // (FLAT backward: 128 pairs of double partials, then the pair of totals)
                const int64_t need = route == 2 ? (int64_t)(2 * 128 + 2) * 8 : (int64_t)nb * C * 3 * 4;
                CHECK(vo_bn_workspace_size(M, C) >= need);
              }
            }
  // the workspace size in closed form: max(ceil(M / RB), 128) row blocks of 3 values per channel, RB = 8192 rows and
  // doubles at C = 1, 512 rows and floats otherwise
  for (int M : Ms)
    for (int C : Cs) {
      const int64_t RB = C == 1 ? 8192 : 512, nb = (M + RB - 1) / RB;
      CHECK(vo_bn_workspace_size(M, C) == (nb > 128 ? nb : 128) * C * 3 * (C == 1 ? 8 : 4));
    }
  // clamped copies, a null record, refused arguments
  int32_t rec[12];
  for (int i = 0; i < 12; ++i) rec[i] = 7;
  CHECK(vo_bn_route(64, 512, VO_BF16, -1, nullptr, nullptr, nullptr, rec, 3) == 3 && rec[2] == 64 && rec[3] == 7);
  CHECK(vo_bn_route(64, 512, VO_BF16, -1, nullptr, nullptr, nullptr, rec, 64) == VO_BN_ROUTE_FIELDS && rec[8] == 7);
  CHECK(vo_bn_route(64, 512, VO_BF16, -1, nullptr, nullptr, nullptr, rec, -5) == 0 && rec[0] == 1);
  CHECK(vo_bn_route(64, 512, VO_BF16, -1, nullptr, nullptr, nullptr, nullptr, 8) == 0);
  CHECK(vo_bn_route(0, 512, VO_BF16, -1, nullptr, nullptr, nullptr, rec, 8) == -1 && rec[0] == 0 && rec[7] == 0);
  CHECK(vo_bn_route(64, -1, VO_BF16, -1, nullptr, nullptr, nullptr, rec, 8) == -1);
  CHECK(vo_bn_route(64, 512, 9, -1, nullptr, nullptr, nullptr, rec, 8) == -1);
  CHECK(vo_bn_route(64, 512, VO_F32, 9, nullptr, nullptr, nullptr, nullptr, 8) == -1);
  std::printf("bn_route_host_check: %ld plans ok\n", plans);
  return 0;
}
