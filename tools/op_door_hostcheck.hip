// Host-side check of what the kernel-level doors do before their first HIP call (vosk_tts_amd/csrc/op_door.hip.h: op_items_check; the
// host-only identity paths of vits_op_resample and vits_op_pitch_shift), which needs no device.  A stand-alone program: build it with
// the host sanitizers and run it,
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/op_door_hostcheck.hip -o tools/op_door_hostcheck && tools/op_door_hostcheck
//
// lengths, x and y live in heap blocks of exactly the size the contract states -- B values, B * N floats -- so a read or a write beyond
// them lands in the sanitizer's red zone.  Not part of the test suite: nothing here touches the GPU, and nothing is loaded into Python.
#include "../vosk_tts_amd/csrc/engine.hip"

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }  // (the HIP runtime's own start-up allocations)

static int g_checks = 0, g_bad = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(c)) { ++g_bad; printf("FAILED line %d: %s\n", __LINE__, #c); }     \
  } while (0)

// a heap block of exactly n values
template <typename T>
struct Block {
  T* p;
  explicit Block(size_t n) : p(static_cast<T*>(malloc(n * sizeof(T)))) {}
  ~Block() { free(p); }
};

static void check_items(int B, long long N, size_t x_elems) {
  Block<float> x(x_elems);
  Block<int64_t> len(B);
  std::vector<int> len32;
  for (int b = 0; b < B; ++b) len.p[b] = b == B - 1 ? N : (N * b) / B;  // 0 first (B > 1), N last
  CHECK(op_items_check("door", x.p, len.p, B, N, &len32) == VITS_OK && (int)len32.size() == B);
  for (int b = 0; b < B; ++b) CHECK(len32[b] == (int)len.p[b]);
  // the first bad item is the one named, and nothing behind it is read as a length of the call
  for (int bad = 0; bad < B; ++bad)
    for (long long v : {-1LL, N + 1}) {
      const int64_t keep = len.p[bad];
      len.p[bad] = v;
      char want[128];
      snprintf(want, sizeof want, "door: length %lld of item %d outside [0, N = %lld]", v, bad, N);
      CHECK(op_items_check("door", x.p, len.p, B, N, &len32, "N = ") == VITS_ERR_ARG && !strcmp(vits_last_error(), want));
      len.p[bad] = keep;
    }
  // refused on B and N alone: neither array is read (null is as good as any)
  CHECK(op_items_check("door", nullptr, len.p, B, N, &len32) == VITS_ERR_ARG && !strcmp(vits_last_error(), "door: bad argument"));
  CHECK(op_items_check("door", x.p, nullptr, B, N, &len32) == VITS_ERR_ARG);
  CHECK(op_items_check("door", x.p, len.p, 0, N, &len32) == VITS_ERR_ARG);
  CHECK(op_items_check("door", x.p, len.p, 65536, N, &len32) == VITS_ERR_ARG);
  CHECK(op_items_check("door", x.p, len.p, B, 0, &len32) == VITS_ERR_ARG);
  CHECK(op_items_check("door", x.p, len.p, B, 1LL << 31, &len32) == VITS_ERR_ARG);
}

// the identity of a door: y[b] = x[b, :len] then zeros, x beyond each length never read into y
template <typename Door>
static void check_identity(int B, long long N, Door door) {
  Block<float> x((size_t)B * N), y((size_t)B * N);
  Block<int64_t> len(B);
  for (int b = 0; b < B; ++b) len.p[b] = b == B - 1 ? N : (N * b) / B;
  for (size_t i = 0; i < (size_t)B * N; ++i) { x.p[i] = (float)(i % 97) - 48.f; y.p[i] = NAN; }
  for (int b = 0; b < B; ++b)
    for (long long i = len.p[b]; i < N; ++i) x.p[(size_t)b * N + i] = NAN;
  CHECK(door(x.p, len.p, B, N, y.p) == VITS_OK);
  for (int b = 0; b < B; ++b)
    for (long long i = 0; i < N; ++i) CHECK(y.p[(size_t)b * N + i] == (i < len.p[b] ? x.p[(size_t)b * N + i] : 0.f));
}

int main() {
  for (int B : {1, 3})
    for (long long N : {1LL, 7LL, 512LL, (1LL << 31) - 1}) check_items(B, N, N > 512 ? 1 : (size_t)B * N);  // (x is never read)
  check_items(65535, 7, (size_t)65535 * 7);
  for (int B : {1, 3})
    for (long long N : {1LL, 7LL, 512LL}) {
      check_identity(B, N, [](const float* x, const int64_t* len, int B_, long long N_, float* y) { return vits_op_resample(0, x, len, B_, N_, 16000, 16000, y); });
      check_identity(B, N, [](const float* x, const int64_t* len, int B_, long long N_, float* y) { return vits_op_pitch_shift(0, x, len, B_, N_, 0.f, y); });
      check_identity(B, N, [](const float* x, const int64_t* len, int B_, long long N_, float* y) { return vits_op_pitch_shift_formant(0, x, len, B_, N_, 0.f, y); });
    }
  // the refusals that stay host-only next to the identity
  {
    Block<float> x(8), y(8);
    Block<int64_t> len(1);
    len.p[0] = 8;
    CHECK(vits_op_pitch_stretch(0, x.p, len.p, 1, 8, 0.f, y.p) == VITS_ERR_ARG && strstr(vits_last_error(), "there is no stretch to return"));
    CHECK(vits_op_pitch_formant_gain(0, x.p, len.p, 1, 8, 0.f, y.p) == VITS_ERR_ARG && strstr(vits_last_error(), "there is no gain to return"));
    double ghz[1];
    CHECK(vits_debug_clock_probe(0, 1000, ghz, 0) == -VITS_ERR_ARG);
  }
  printf("op_door_hostcheck: %d checks, %d failed\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
