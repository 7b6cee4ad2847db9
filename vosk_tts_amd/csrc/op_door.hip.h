// op_door.hip.h -- the scaffold of a kernel-level parity entry point ("door"): host buffers in, one kernel family, host buffers out, no
// model and no session.  DevBufs owns the device buffers of one call; OpDoor is the call itself: begin on a device, upload, NaN-filled
// outputs, finish (last error + device synchronise), download, one return code.  A door reads: check, scope, up / out, launch, finish,
// down, return rc.  Part of the ONE translation unit engine.hip (included there, ahead of resample.hip.h; not a standalone header).
#pragma once

// device buffers owned by one call, freed with it
struct DevBufs {
  std::vector<void*> bufs;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() { for (void* p : bufs) hipFree(p); }
  void* operator()(size_t bytes) {  // null: the allocation failed
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    bufs.push_back(p);
    return p;
  }
  void release(void* p) { bufs.erase(std::remove(bufs.begin(), bufs.end(), p), bufs.end()); }  // p outlives the call: the caller's now
};

// A table that lives as long as the process: src[0 .. bytes) to a fresh allocation on `device`, *d (null on failure).  hipMalloc and a
// synchronous copy: call it outside stream capture.  `what` is the stage's name in the two messages.
static int dev_table_upload(int device, const char* what, const void* src, size_t bytes, void** d) {
  *d = nullptr;
  HIP_TRY(hipSetDevice(device));
  if (hipMalloc(d, bytes) != hipSuccess) { *d = nullptr; return fail(VITS_ERR_NOMEM, "%s: table alloc failed", what); }
  if (hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(*d);
    *d = nullptr;
    return fail(VITS_ERR_DEVICE, "%s: table upload failed", what);
  }
  return VITS_OK;
}

// The tables of a stage that live as long as the process, by key (the device, and whatever else tells two tables apart).  get() leaves
// *out at the entry of `key`; on a miss build(Val&) fills a fresh one under the lock (dev_table_upload: outside stream capture).  What
// build refuses is not kept, and nothing is ever evicted: captured graphs and cached contexts hold the pointers.
template <typename Key, typename Val>
struct DevTabs {
  std::mutex mu;
  std::map<Key, Val> tabs;
  size_t size() const { return tabs.size(); }  // (for a build that bounds the table count: it runs under the lock)
  template <typename Build>
  int get(const Key& key, const Val** out, Build&& build) {
    std::lock_guard<std::mutex> g(mu);
    auto it = tabs.find(key);
    if (it == tabs.end()) {
      Val v{};
      TRY(build(v));
      it = tabs.emplace(key, v).first;
    }
    *out = &it->second;
    return VITS_OK;
  }
};

// One door call on the null stream.  The first failure is kept (fail() has its message, under the door's name) and every later step is
// skipped; a door guards its launches with ok().  A failed allocation is VITS_ERR_NOMEM, any other HIP error VITS_ERR_DEVICE.
struct OpDoor {
  const char* what;
  DevBufs bufs;
  int code = VITS_OK;
  OpDoor(const char* what_, int device) : what(what_) { hip(hipSetDevice(device)); }
  bool ok() const { return code == VITS_OK; }
  int rc() const { return code; }
  void hip(hipError_t e) {
    if (ok() && e != hipSuccess) code = fail(VITS_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  template <typename T>
  T* dev(size_t n) {  // n elements, not initialised
    if (!ok()) return nullptr;
    T* p = static_cast<T*>(bufs(n * sizeof(T)));
    if (!p) code = fail(VITS_ERR_NOMEM, "%s: device alloc failed (%zu bytes)", what, n * sizeof(T));
    return p;
  }
  template <typename T>
  T* up(const T* host, size_t n) {  // the device copy of host[0 .. n); a null host pointer gives a null device pointer
    T* p = host ? dev<T>(n) : nullptr;
    if (p) hip(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  // x [B, N] as a zero-filled [B, N] on the device with every item's own samples only: what lies at and beyond lengths[b] never gets there
  float* up_items(const float* x, const int64_t* lengths, int B, int64_t N) {
    float* dx = out<float>((size_t)B * N, 0);
    for (int b = 0; b < B && ok(); ++b)
      if (lengths[b]) hip(hipMemcpy(dx + (size_t)b * N, x + (size_t)b * N, sizeof(float) * (size_t)lengths[b], hipMemcpyHostToDevice));
    return dx;
  }
  template <typename T>
  T* out(size_t n, int fill = 0xff) {  // 0xff: an element the kernel does not write shows as NaN
    T* p = dev<T>(n);
    if (p) hip(hipMemset(p, fill, n * sizeof(T)));
    return p;
  }
  void finish() {  // behind the launches
    hip(hipGetLastError());
    hip(hipDeviceSynchronize());
  }
  template <typename T>
  void down(T* host, const T* d, size_t n) {
    if (ok()) hip(hipMemcpy(host, d, n * sizeof(T), hipMemcpyDeviceToHost));
  }
};

// what the doors over B items x [B, N] on the host check first; len32: the lengths as the kernels take them.  `what` is the door's name
// in its messages, `n_name` what it calls N there.
static int op_items_check(const char* what, const float* x, const int64_t* lengths, int32_t B, int64_t N, std::vector<int>* len32,
                          const char* n_name = "") {
  if (!x || !lengths || B <= 0 || B > 65535 || N <= 0 || N >= (1LL << 31)) return fail(VITS_ERR_ARG, "%s: bad argument", what);
  len32->resize(B);
  for (int b = 0; b < B; ++b) {
    if (lengths[b] < 0 || lengths[b] > N)
      return fail(VITS_ERR_ARG, "%s: length %lld of item %d outside [0, %s%lld]", what, (long long)lengths[b], b, n_name, (long long)N);
    (*len32)[b] = (int)lengths[b];
  }
  return VITS_OK;
}
