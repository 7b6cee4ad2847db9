// Host-side check of the fast paths' two caches (vosk_tts_amd/csrc/ctx_cache.hip.h: IdleCache, LruSlots), which need no device and
// no HIP.  A stand-alone program: build it twice with the host sanitizers and run both,
//
//   c++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/ctx_cache_hostcheck.cpp -o tools/ctx_cache_hostcheck && tools/ctx_cache_hostcheck
//   c++ -O1 -g -std=c++17 -pthread -fsanitize=thread tools/ctx_cache_hostcheck.cpp -o tools/ctx_cache_hostcheck && tools/ctx_cache_hostcheck
//
// The contexts are plain heap objects counted on new and delete: a victim handed back twice is a double free for the address
// sanitizer, one never handed back leaves the counter above zero.  Not part of the test suite: nothing here touches the GPU, and
// nothing is loaded into Python.
#include "../vosk_tts_amd/csrc/ctx_cache.hip.h"

#include <stdio.h>

#include <atomic>
#include <thread>

static int g_checks = 0, g_bad = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(c)) { ++g_bad; printf("FAILED line %d: %s\n", __LINE__, #c); }     \
  } while (0)

static std::atomic<int> g_live{0};
struct Ctx {
  int id;
  explicit Ctx(int id_) : id(id_) { ++g_live; }
  ~Ctx() { --g_live; }
};
static void free_all(const std::vector<Ctx*>& v) { for (Ctx* c : v) delete c; }

static size_t g_byte_cap = 0;
static size_t byte_cap() { return g_byte_cap; }

// count cap: after cap + k distinct keys exactly k victims came back, in order of first use
static void idle_count_cap(size_t cap, bool keep_duplicates) {
  std::mutex mu;
  IdleCache<int, Ctx> C(mu, {cap, keep_duplicates});
  const int k = 5;
  std::vector<int> victims;
  for (int i = 0; i < (int)cap + k; ++i)
    for (Ctx* v : C.put(i, new Ctx(i), 0)) { victims.push_back(v->id); delete v; }
  CHECK((int)victims.size() == k && C.size() == cap);
  for (int i = 0; i < (int)victims.size(); ++i) CHECK(victims[i] == i);
  // a take and a put make the oldest the newest: the second-oldest goes next
  Ctx* c = C.take(k);
  CHECK(c && c->id == k && C.size() == cap - 1);
  CHECK(C.take(0) == nullptr);
  CHECK(C.put(k, c, 0).empty());
  std::vector<Ctx*> v = C.put(1000, new Ctx(1000), 0);
  CHECK(v.size() == 1 && v[0]->id == k + 1);
  free_all(v);
  v = C.take_all();
  CHECK(v.size() == cap && C.size() == 0 && C.take_all().empty());
  free_all(v);
  CHECK(g_live == 0);
}

static void slots_count_cap(size_t cap) {
  LruSlots<int, Ctx> S;
  const int k = 5;
  std::vector<int> victims;
  auto add = [&](int key) {
    CHECK(S.find(key) == nullptr);
    if (Ctx* v = S.make_room(cap)) { victims.push_back(v->id); delete v; }
    S.insert(key, new Ctx(key));
  };
  for (int i = 0; i < (int)cap + k; ++i) add(i);
  CHECK((int)victims.size() == k && S.size() == cap);
  for (int i = 0; i < (int)victims.size(); ++i) CHECK(victims[i] == i);
  // find touches: use the oldest entry and the second-oldest becomes the victim
  Ctx* c = S.find(k);
  CHECK(c && c->id == k);
  victims.clear();
  add(1000);
  CHECK(victims.size() == 1 && victims[0] == k + 1 && S.find(k) == c);
  int seen = 0;
  S.for_each([&](const Ctx&) { ++seen; });
  CHECK(seen == (int)cap);
  std::vector<Ctx*> v = S.drain();
  CHECK(v.size() == cap && S.size() == 0 && S.drain().empty() && S.make_room(cap) == nullptr && S.make_room(0) == nullptr);
  free_all(v);
  CHECK(g_live == 0);
}

// byte cap: over budget, victims are returned until under it, or until one remains
static void idle_byte_cap() {
  std::mutex mu;
  IdleCache<int, Ctx> C(mu, {48, true, byte_cap});
  g_byte_cap = 100;
  CHECK(C.put(0, new Ctx(0), 40).empty());
  CHECK(C.put(1, new Ctx(1), 40).empty());
  std::vector<Ctx*> v = C.put(2, new Ctx(2), 40);  // 120 > 100: the oldest goes, 80 stay
  CHECK(v.size() == 1 && v[0]->id == 0 && C.size() == 2);
  free_all(v);
  v = C.put(3, new Ctx(3), 90);  // 170: 1 and 2 go, 90 stay
  CHECK(v.size() == 2 && v[0]->id == 1 && v[1]->id == 2 && C.size() == 1);
  free_all(v);
  v = C.put(4, new Ctx(4), 500);  // alone above the cap: everything else goes, this one stays
  CHECK(v.size() == 1 && v[0]->id == 3 && C.size() == 1);
  free_all(v);
  Ctx* c = C.take(4);  // a take gives its bytes back
  CHECK(c && c->id == 4 && C.size() == 0);
  CHECK(C.put(5, new Ctx(5), 100).empty());
  g_byte_cap = 0;  // (VITS_CACHE_MB=0): one idle context survives a release
  v = C.put(4, c, 500);
  CHECK(v.size() == 1 && v[0]->id == 5 && C.size() == 1);
  free_all(v);
  free_all(C.take_all());
  CHECK(g_live == 0);
}

static void idle_duplicates() {
  std::mutex mu;
  {
    IdleCache<int, Ctx> C(mu, {48, true});
    CHECK(C.put(7, new Ctx(1), 0).empty() && C.put(7, new Ctx(2), 0).empty() && C.size() == 2);
    Ctx *a = C.take(7), *b = C.take(7);
    CHECK(a && b && a != b && C.take(7) == nullptr);
    delete a; delete b;
  }
  {
    IdleCache<int, Ctx> C(mu, {16, false});
    CHECK(C.put(7, new Ctx(1), 0).empty());
    std::vector<Ctx*> v = C.put(7, new Ctx(2), 0);
    CHECK(v.size() == 1 && v[0]->id == 1 && C.size() == 1);
    free_all(v);
    Ctx* a = C.take(7);
    CHECK(a && a->id == 2 && C.take(7) == nullptr);
    delete a;
  }
  CHECK(g_live == 0);
}

// 8 threads doing take-or-create / put on 3 keys with a cap of 2: afterwards live count = idle count <= cap
static void idle_threads(bool keep_duplicates) {
  std::mutex mu;
  IdleCache<int, Ctx> C(mu, {2, keep_duplicates});
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&C, t] {
      for (int i = 0; i < 2000; ++i) {
        const int key = (t + i) % 3;
        Ctx* c = C.take(key);
        if (!c) c = new Ctx(key);
        c->id = key;  // (the holder writes its context: a context shared by two threads is a race for the thread sanitizer)
        free_all(C.put(key, c, 1));
      }
    });
  for (auto& x : th) x.join();
  CHECK((size_t)g_live == C.size() && C.size() <= 2);
  free_all(C.take_all());
  CHECK(g_live == 0);
}

int main() {
  for (size_t cap : {48, 16, 6, 4}) {
    idle_count_cap(cap, true);
    idle_count_cap(cap, false);
    slots_count_cap(cap);
  }
  idle_byte_cap();
  idle_duplicates();
  idle_threads(true);
  idle_threads(false);
  printf("ctx_cache_hostcheck: %d checks, %d failed\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
