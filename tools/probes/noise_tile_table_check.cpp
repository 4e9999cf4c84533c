// NoiseTileTable (csrc/fdsr_kernels.h) on the host alone: set / clear, for_call below, at and above n, a cleared table, refused
// arguments.  No GPU, no Python: the table only stores the caller's pointer and never reads through it, so a host array stands in.
// Meant to run under the sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/noise_tile_table_check.cpp -o tools/probes/noise_tile_table_check && tools/probes/noise_tile_table_check
#include <cstdio>
#include <cstdlib>

#include "../../fastdiffsr_amd/csrc/fdsr_kernels.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

using fdsr::NoiseTiles;
using fdsr::NoiseTileTable;

static bool is_plain(const NoiseTiles& t) { return t.origins == nullptr && t.scene_w == 0 && t.W == 0; }

int main() {
  int32_t* origins = new int32_t[3 * 2]{0, 0, 28, 44, 5, 3};
  NoiseTileTable t;
  NoiseTiles call{origins, 7, 7};   // stale on purpose: for_call must overwrite every field

  // a fresh table is a cleared one: every batch fits and addresses by batch position
  EXPECT(t.origins == nullptr && t.n == 0 && t.scene_w == 0);
  EXPECT(t.for_call(1, 32, &call) && is_plain(call));
  EXPECT(t.for_call(1 << 20, 32, &call) && is_plain(call));

  // set, then calls below, at and above n
  EXPECT(t.set(origins, 3, 76));
  EXPECT(t.origins == origins && t.n == 3 && t.scene_w == 76);
  for (int batch = 1; batch <= 3; ++batch) {
    call = NoiseTiles{};
    EXPECT(t.for_call(batch, 32, &call));
    EXPECT(call.origins == origins && call.scene_w == 76 && call.W == 32);
  }
  call = NoiseTiles{origins, 7, 7};
  EXPECT(!t.for_call(4, 32, &call) && is_plain(call));   // refused, and nothing of the table leaks into the call
  EXPECT(t.n == 3);                                      // what the refusal's message names

  // bad arguments: refused, and the table that was set stays as it is
  EXPECT(!t.set(origins, 0, 76));
  EXPECT(!t.set(origins, 3, 0));
  EXPECT(!t.set(origins, -1, 76));
  EXPECT(!t.set(origins, 3, -5));
  EXPECT(t.origins == origins && t.n == 3 && t.scene_w == 76);

  // clearing stores zeros whatever the counts say, and a cleared table takes every call
  EXPECT(t.set(nullptr, 9, 99));
  EXPECT(t.origins == nullptr && t.n == 0 && t.scene_w == 0);
  call = NoiseTiles{origins, 7, 7};
  EXPECT(t.for_call(4, 32, &call) && is_plain(call));
  EXPECT(t.set(nullptr, 0, 0));
  EXPECT(!t.set(origins, 0, 0) && t.origins == nullptr);   // a refused set on a cleared table leaves it cleared

  delete[] origins;   // the table never owned it; the sanitizers see the one allocation released
  std::puts("noise_tile_table_check: ok");
  return 0;
}
