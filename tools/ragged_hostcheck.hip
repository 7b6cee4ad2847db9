// Host-side check of the batch descriptor of the output tail (vosk_tts_amd/csrc/ragged.hip.h: Items, n_out) and of the two rules stated
// through n_out (marks_end of marks.hip.h, ResamplePlan::n_out of resample.hip.h), which are __host__ __device__ and need no device.  A
// stand-alone program, built and run the way tools/out_tail_hostcheck.hip is:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/ragged_hostcheck.hip -o tools/ragged_hostcheck && tools/ragged_hostcheck
//
// (tests/test_ragged_items.py builds it without the sanitizers and runs it.)  Every length is compared with a restatement in 128-bit
// integers that shares no code with the header.  Nothing here touches the GPU, and nothing is loaded into Python.
#include "../vosk_tts_amd/csrc/engine.hip"

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }  // (the HIP runtime's own start-up allocations)

static int g_checks = 0, g_bad = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(c)) { ++g_bad; printf("FAILED line %d: %s\n", __LINE__, #c); }     \
  } while (0)

typedef __int128 wide;
static wide ceil_div(wide a, wide b) { return (a + b - 1) / b; }  // a >= 0, b > 0

int main() {
  const int units[] = {0, 1, 7, 4000000, 2147483647 / 512};  // (the last: the longest item whose samples still fit 2^31 at hop 512)
  const int B = (int)(sizeof(units) / sizeof(units[0]));
  const long long muls[] = {1, 256, 512};
  const int rates[][2] = {{1, 1}, {160, 441}, {320, 147}, {4, 1}};
  for (long long mul : muls)
    for (const auto& r : rates) {
      const int L = r[0], M = r[1];
      for (int with_units = 0; with_units < 2; ++with_units)
        for (int b = 0; b < B; ++b) {
          const wide in = with_units ? (wide)units[b] * mul : (wide)mul;
          const wide out = ceil_div(in * L, M);
          CHECK((wide)n_out((long long)in, L, M) == out);
          for (long long cap : {(long long)out - 1, (long long)out, (long long)out + 1, 0LL, 1LL << 40}) {  // below, at, above the unclamped value
            if (cap < 0) continue;
            const Items it{with_units ? units : nullptr, mul, L, M, cap};
            CHECK((wide)it.len_in(b) == in);
            CHECK((wide)it.len_out(b) == (out < cap ? out : (wide)cap));
            for (int b0 = 0; b0 <= b; ++b0) {  // the same batch from item b0 on: item b is its item b - b0
              const Items g = it.from(b0);
              CHECK(g.mul == it.mul && g.L == it.L && g.M == it.M && g.cap == it.cap && (g.units == nullptr) == (it.units == nullptr));
              CHECK(g.len_in(b - b0) == it.len_in(b) && g.len_out(b - b0) == it.len_out(b));
            }
          }
          // the two rules stated through n_out, on the same grid
          if (with_units) CHECK((wide)marks_end(units[b], mul, L, M) == out);
          ResamplePlan P;
          P.L = L; P.M = M;
          CHECK((wide)P.n_out((long long)in) == out);
        }
    }
  // the helper behind every caller: a null table is the native rate
  ResampleTab T;
  CHECK(resample_plan(22050, 8000, &T.P) == VITS_OK);
  const Items a = items_at(&T, units, 256, 99), n = items_at(nullptr, units, 256, 99);
  CHECK(a.L == 160 && a.M == 441 && a.units == units && a.mul == 256 && a.cap == 99);
  CHECK(n.L == 1 && n.M == 1 && n.units == units && n.mul == 256 && n.cap == 99);
  const Items v{units, 1};  // the form the contour stage hands its vlen array over in
  CHECK(v.L == 1 && v.M == 1 && v.len_in(2) == 7);

  printf("ragged_hostcheck: %d checks, %d failed\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
