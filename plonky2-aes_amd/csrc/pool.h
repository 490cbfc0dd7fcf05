// Workspaces that concurrent callers of one handle lease for the length of a call: one pool and one lease for the prover's
// staging sets, the verification workspaces and the witness workspaces (prover_gpu.hip).  Nothing here knows HIP.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

struct NoKey {  // a pool whose workspaces never go stale
    bool operator==(NoKey) const { return true; }
};

// Free workspaces and the key new ones are made under (a chunk option).  W has a member `key`: what it was made under.
template <class W, class Key = size_t>
class Pool {
    std::mutex mu;
    std::vector<std::unique_ptr<W>> free_;
    Key key_;

public:
    explicit Pool(Key k = Key{}) : key_(k) {}
    void set_key(Key k) {
        std::lock_guard<std::mutex> lock(mu);
        key_ = k;
    }
    size_t idle() {  // for tests/host/pool_check.cpp; the product never asks
        std::lock_guard<std::mutex> lock(mu);
        return free_.size();
    }
    // A free workspace of the current key, else make(key) (null or an exception: the pool is as it was).  Workspaces made under
    // an older key go on the way; their destructors wait for their last users, so they run after the lock is released.
    template <class Make>
    std::unique_ptr<W> lease(Make&& make) {
        std::vector<std::unique_ptr<W>> stale;
        std::unique_ptr<W> w;
        Key k;
        {
            std::lock_guard<std::mutex> lock(mu);
            k = key_;
            while (!free_.empty() && !w) {
                w = std::move(free_.back());
                free_.pop_back();
                if (!(w->key == k)) stale.push_back(std::move(w));
            }
        }
        stale.clear();
        return w ? std::move(w) : make(k);
    }
    void give(std::unique_ptr<W> w) {
        std::lock_guard<std::mutex> lock(mu);
        free_.push_back(std::move(w));
    }
};

// The workspace goes back to its pool on every way out of a call.  Until the call sets failed = false, what it enqueued may
// still be using the workspace: W::drain(has_caller, caller) waits for the caller's stream (device forms: on_stream; a stream
// is an opaque pointer here, as in the C ABI, and null is a stream too) and for the workspace's own before the next lease.
template <class W, class Key = size_t>
struct Lease {
    Pool<W, Key>& pool;
    std::unique_ptr<W> ws;
    void* caller = nullptr;
    bool has_caller = false, failed = true;
    void on_stream(void* s) { caller = s, has_caller = true; }
    template <class Make>
    Lease(Pool<W, Key>& p, Make&& make) : pool(p), ws(p.lease(make)) {}
    Lease(const Lease&) = delete;
    ~Lease() {
        if (!ws) return;
        if (failed) ws->drain(has_caller, caller);
        pool.give(std::move(ws));
    }
    W* operator->() const { return ws.get(); }
    explicit operator bool() const { return (bool)ws; }
};
