// ctx_cache.hip.h -- the two caches of the graph-replayed fast paths (engine_fastpath.hip.h, stts.hip.h), written once.
// Host-only C++: no HIP call and no HIP include, so tools/ctx_cache_hostcheck.cpp includes this file alone.  Neither cache frees
// anything: a context that has to go is handed back to the caller, which knows what it owns and frees it outside any lock.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <vector>

// ---- the caps, named once
enum : size_t {
  VITS_FRONTS_PER_MODEL = 48,  // (or IdlePolicy::byte_cap, whichever is reached first)
  VITS_BACKS_PER_FRONT = 6,    // frame buckets per T_x bucket; vosk_tts_amd/session.py BACK_SESSIONS_PER_FRONT mirrors this value (warmup plans with it)
  VITS_RATES_PER_BACK = 4,     // output rates per frame bucket
  STTS_FRONTS_PER_MODEL = 16,
  STTS_BACKS_PER_FRONT = 4,    // (frame bucket, n_steps) pairs per T_x bucket
};

struct IdlePolicy {
  size_t count_cap;
  bool keep_duplicates;            // a second idle context of one key: kept next to the first (VITS) or put in its place (StableTTS)
  size_t (*byte_cap)() = nullptr;  // null: no cap on bytes.  Asked by put, never before the first one; at least one context stays whatever it says
};

// the entry of a non-empty map with the smallest stamp (stamps of one cache are distinct: its clock gives each use the next one)
template <typename Map>
static typename Map::iterator ctx_lru(Map& m) {
  auto lru = m.begin();
  for (auto it = m.begin(); it != m.end(); ++it)
    if (it->second.stamp < lru->second.stamp) lru = it;
  return lru;
}

// Idle cache: the contexts of one model that no call is using, by key, least recently used out first.  A call takes one out for its
// whole length and puts it back at its end, so two threads never share a context.  `mu` is the owner's mutex (vits_model::pool_mu).
template <typename Key, typename Ctx>
class IdleCache {
  struct Ent { Ctx* ctx; size_t bytes; uint64_t stamp; };
  std::mutex& mu_;
  const IdlePolicy pol_;
  std::multimap<Key, Ent> idle_;
  uint64_t clock_ = 0;
  size_t bytes_ = 0;

 public:
  IdleCache(std::mutex& mu, const IdlePolicy& pol) : mu_(mu), pol_(pol) {}
  Ctx* take(const Key& key) {  // an idle context of `key`, now the caller's; null: none
    std::lock_guard<std::mutex> g(mu_);
    auto it = idle_.find(key);
    if (it == idle_.end()) return nullptr;
    Ctx* c = it->second.ctx;
    bytes_ -= it->second.bytes;
    idle_.erase(it);
    return c;
  }
  // `ctx` (pinning `bytes`) is idle from now on and the most recently used; returns the contexts that had to go for it
  std::vector<Ctx*> put(const Key& key, Ctx* ctx, size_t bytes) {
    std::vector<Ctx*> out;
    std::lock_guard<std::mutex> g(mu_);
    auto drop = [&](typename std::multimap<Key, Ent>::iterator it) {
      bytes_ -= it->second.bytes;
      out.push_back(it->second.ctx);
      idle_.erase(it);
    };
    if (!pol_.keep_duplicates) {
      auto it = idle_.find(key);
      if (it != idle_.end()) drop(it);  // a concurrent call built the same key: keep the newer
    }
    idle_.emplace(key, Ent{ctx, bytes, ++clock_});
    bytes_ += bytes;
    const size_t byte_cap = pol_.byte_cap ? pol_.byte_cap() : SIZE_MAX;
    while ((bytes_ > byte_cap && idle_.size() > 1) || idle_.size() > pol_.count_cap) drop(ctx_lru(idle_));
    return out;
  }
  std::vector<Ctx*> take_all() {
    std::vector<Ctx*> out;
    std::lock_guard<std::mutex> g(mu_);
    for (auto& kv : idle_) out.push_back(kv.second.ctx);
    idle_.clear();
    bytes_ = 0;
    return out;
  }
  size_t size() {
    std::lock_guard<std::mutex> g(mu_);
    return idle_.size();
  }
};

// LRU slots: the children one checked-out context owns (backs of a front, rates of a back).  Only the call that holds the parent
// touches them, so there is no lock.  The caller frees what make_room / drain hand back -- after waiting for the parent's stream.
template <typename Key, typename Ctx>
class LruSlots {
  struct Ent { Ctx* ctx; uint64_t stamp; };
  std::map<Key, Ent> m_;
  uint64_t clock_ = 0;

 public:
  Ctx* find(const Key& key) {  // a hit is a use
    auto it = m_.find(key);
    if (it == m_.end()) return nullptr;
    it->second.stamp = ++clock_;
    return it->second.ctx;
  }
  Ctx* make_room(size_t cap) {  // before an insert: with `cap` slots taken, the least recently used leaves and is returned
    if (m_.size() < cap || m_.empty()) return nullptr;
    auto lru = ctx_lru(m_);
    Ctx* c = lru->second.ctx;
    m_.erase(lru);
    return c;
  }
  void insert(const Key& key, Ctx* ctx) { m_[key] = Ent{ctx, ++clock_}; }  // (of a key that find did not have)
  std::vector<Ctx*> drain() {
    std::vector<Ctx*> out;
    for (auto& kv : m_) out.push_back(kv.second.ctx);
    m_.clear();
    return out;
  }
  size_t size() const { return m_.size(); }
  template <typename Fn>
  void for_each(Fn fn) const { for (auto& kv : m_) fn(*kv.second.ctx); }
};
