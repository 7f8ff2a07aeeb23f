// dense_geom.cpp — k_small's dense fetch geometry (yustack_amd/csrc/yucsum_dense.h)
// on a CPU: for every step and lane of a set of batches, what is loaded, what is
// not, and where each group finds its window in the wave's LDS slice. Addresses
// are plain numbers here; nothing is dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "yucsum_dense.h"

namespace {

constexpr int G = 16, U = 6, GPW = 64 / G;
constexpr uint32_t kSlice = yu::kDensePiece * U;

int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++g_fail <= 20) {                            \
        printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        printf(__VA_ARGS__);                           \
        printf("\n");                                  \
      }                                                \
    }                                                  \
  } while (0)

bool ok(uint64_t data, uint64_t stride, uint32_t len, bool fill = false, bool ipv4 = false,
        bool ragged = false) {
  return yu::dense_ok(G, U, data, ragged, stride, len, fill, ipv4);
}

void check_step(uint64_t data, uint32_t len, uint64_t n, uint64_t pb) {
  const uint64_t end = data + n * len;           // one past the batch's last byte
  const uint64_t dend = (end + 3u) & ~3ull;      // the descriptor's end (rsrc_at)
  const yu::DenseStep s = yu::dense_step(data, len, n, pb, GPW);
  const uint64_t start = data + pb * len;
  CHECK(s.base % 128 == 0 && s.base <= start && start - s.base < 128 && s.base + s.lead == start,
        "len %u n %llu pb %llu", len, (unsigned long long)n, (unsigned long long)pb);
  const uint64_t npk = pb >= n ? 0 : (n - pb < (uint64_t)GPW ? n - pb : GPW);
  // bytes of the slice image that loads fill: count per byte
  std::vector<int> cover(kSlice, 0);
  for (uint32_t u = 0; u < (uint32_t)U; ++u) {
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t off = yu::dense_chunk(s, u, lane);
      const uint32_t nominal = yu::kDensePiece * u + 16u * lane;
      if (off == yu::kDenseOOB) continue;
      CHECK(npk != 0, "a load for pb >= n: len %u n %llu pb %llu", len, (unsigned long long)n,
            (unsigned long long)pb);
      CHECK(off == nominal, "lane %u load %u at %u", lane, u, off);
      const uint64_t a = s.base + off;
      // inside [data, ceil4(end)): the range check is per dword, so the chunk
      // holding the end is cut there; its first dword must be inside
      CHECK(a >= data && a + 4 <= dend, "chunk %llu outside [%llu, %llu)", (unsigned long long)a,
            (unsigned long long)data, (unsigned long long)dend);
      // nothing for a packet >= n: the chunk begins before the batch's end
      CHECK(a < end, "chunk %llu at or past the end %llu", (unsigned long long)a,
            (unsigned long long)end);
      // only lines the step's packets touch
      CHECK(off / 128 <= (s.lead + (uint32_t)npk * len - 1) / 128, "chunk %u past the step's last line",
            off);
      for (uint32_t b = 0; b < 16 && a + b < dend; ++b) cover[off + b]++;
    }
  }
  // every byte of every packet of the step exactly once
  for (uint64_t b = 0; b < npk * len; ++b)
    CHECK(cover[s.lead + b] == 1, "byte %llu of step pb %llu covered %d times (len %u n %llu)",
          (unsigned long long)b, (unsigned long long)pb, cover[s.lead + b], len, (unsigned long long)n);
  // whole lines: before the batch's last step, every chunk of a touched line
  // that lies in the batch is asked for
  if (npk && pb + GPW < n) {
    const uint32_t last = (s.lead + (uint32_t)npk * len - 1) / 128;
    for (uint32_t x = 0; x < (last + 1) * 128; ++x)
      CHECK(cover[x] == (s.base + x >= data ? 1 : 0), "byte %u of the range covered %d times", x, cover[x]);
  }
  // the groups' windows in the LDS slice
  for (uint32_t gw = 0; gw < (uint32_t)GPW; ++gw) {
    if (pb + gw >= n) continue;  // inactive group: reads nothing it uses
    const uint32_t wo = yu::dense_window(data, len, pb, gw);
    CHECK(s.base + wo == data + (pb + gw) * len, "window of group %u at %u", gw, wo);
    CHECK(wo % 4 == 0, "window %u not dword-aligned", wo);
    CHECK(wo + 16u * G * U <= kSlice + yu::dense_pad(G, U), "window %u leaves the padded slice", wo);
    for (uint32_t u = 0; u < (uint32_t)U; ++u)
      for (uint32_t gl = 0; gl < (uint32_t)G; ++gl) {
        const uint32_t cr = 16u * (gl + u * G);
        // past the slice only where the window path marks the lane out of range
        if (wo + cr + 16u > kSlice) CHECK(cr >= len, "chunk %u of group %u leaves the slice", cr, gw);
      }
  }
}

}  // namespace

int main() {
  const uint32_t lens[] = {1024, 1400, 1496, 1500, 1504, 1528};
  const uint64_t datas[] = {4096 + 0, 4096 + 16, 4096 + 48, 4096 + 112, 4096 + 128};
  const uint64_t ns[] = {1, 3, 4, 5, 17};
  for (uint32_t len : lens)
    for (uint64_t data : datas) {
      const bool fits = (uint64_t)GPW * len + 124 <= kSlice;
      CHECK(ok(data, len, len) == fits, "predicate for len %u data %llu", len, (unsigned long long)data);
      if (!ok(data, len, len)) continue;
      for (uint64_t n : ns) {
        for (uint64_t pb = 0; pb < n; pb += GPW) check_step(data, len, n, pb);
        check_step(data, len, n, n);  // a wave with no next step fetches packet n: nothing
      }
    }
  // config 3's shape takes the path
  CHECK(ok(4096, 1500, 1500), "config 3");
  // and these do not
  CHECK(!ok(4096, 1498, 1498), "len 1498");
  CHECK(!ok(4096 + 4, 1500, 1500), "data & 15 == 4");
  CHECK(!ok(4096, 1504, 1500), "stride != len");
  CHECK(!ok(4096, 1500, 1500, true), "fill");
  CHECK(!ok(4096, 1500, 1500, false, true), "IPv4 mode");
  CHECK(!ok(4096, 1532, 1532), "len 1532");
  CHECK(!ok(4096, 1500, 1500, false, false, true), "ragged");
  CHECK(!yu::dense_ok(16, 4, 4096, false, 1000, 1000, false, false), "another instantiation");
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok\n");
  return 0;
}
