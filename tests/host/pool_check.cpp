// Stand-alone check of csrc/pool.h (tests/test_pool_host.py builds it under the address, undefined-behaviour and thread
// sanitizers): a workspace type that counts its constructions, destructions and drains stands in for the GPU workspaces.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>

#include "pool.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static std::atomic<long> g_made{0}, g_gone{0}, g_drains{0}, g_caller_drains{0};

struct Fake;
static Pool<Fake>* g_pool = nullptr;  // what ~Fake locks: a destructor that ran under the pool's lock would deadlock here
struct Fake {
    size_t key;
    bool alive = true;
    explicit Fake(size_t k) : key(k) { g_made++; }
    Fake(const Fake&) = delete;
    ~Fake() {
        CHECK(alive);  // exactly once
        alive = false;
        if (g_pool) (void)g_pool->idle();
        g_gone++;
    }
    void drain(bool has_caller, void* caller) {
        g_drains++;
        if (has_caller) g_caller_drains += *(int*)caller;
    }
};
static std::unique_ptr<Fake> make(size_t k) { return std::make_unique<Fake>(k); }

static void reuse_and_stale() {
    Pool<Fake> pool(3);
    g_pool = &pool;
    Fake* first;
    {
        Lease<Fake> a(pool, make);
        CHECK(a && a->key == 3 && g_made == 1);
        first = a.ws.get();
        a.failed = false;
    }
    CHECK(pool.idle() == 1 && g_gone == 0 && g_drains == 0);  // returned, and no drain after a success
    {
        Lease<Fake> a(pool, make), b(pool, make);  // the returned one again, and a second for the concurrent caller
        CHECK(a.ws.get() == first && b.ws.get() != first && g_made == 2);
        a.failed = b.failed = false;
    }
    CHECK(pool.idle() == 2 && g_gone == 0);
    pool.set_key(7);
    {
        Lease<Fake> a(pool, make);  // both stale ones go (their destructors take the pool's lock), one of key 7 is made
        CHECK(a->key == 7 && g_made == 3 && g_gone == 2 && pool.idle() == 0);
        a.failed = false;
    }
    CHECK(pool.idle() == 1);
    g_pool = nullptr;
}

static void failing_make() {
    const long made = g_made, gone = g_gone;
    Pool<Fake> pool(1);
    {
        Lease<Fake> a(pool, make);
        a.failed = false;
    }
    pool.set_key(1);
    {
        Lease<Fake> a(pool, make), none(pool, [](size_t) { return std::unique_ptr<Fake>(); });  // the free one is out: make runs
        CHECK(a && !none);
        a.failed = false;
    }  // (a lease without a workspace returns nothing)
    CHECK(pool.idle() == 1 && g_made == made + 1 && g_gone == gone);
    bool thrown = false;
    try {
        Lease<Fake> a(pool, make);
        a.failed = false;
        Lease<Fake> b(pool, [](size_t) -> std::unique_ptr<Fake> { throw std::runtime_error("out of memory"); });
    } catch (std::runtime_error&) {
        thrown = true;
    }
    CHECK(thrown && pool.idle() == 1 && g_made == made + 1 && g_gone == gone);
}

static void drains() {
    Pool<Fake> pool(1);
    const long d0 = g_drains;
    { Lease<Fake> a(pool, make); }  // never marked as succeeded: drained, with no caller's stream
    CHECK(g_drains == d0 + 1 && g_caller_drains == 0 && pool.idle() == 1);
    int stream = 5;  // what a stream handle points to
    {
        Lease<Fake> a(pool, make);
        a.on_stream(&stream);  // a device form: the caller's stream is drained as well
    }
    CHECK(g_drains == d0 + 2 && g_caller_drains == 5 && pool.idle() == 1);
    {
        Lease<Fake> a(pool, make);
        a.on_stream(&stream);
        a.failed = false;
    }
    CHECK(g_drains == d0 + 2 && g_caller_drains == 5);
}

static void threads() {
    const long made = g_made, gone = g_gone;
    {
        Pool<Fake> pool(0);
        g_pool = &pool;
        std::atomic<bool> stop{false};
        std::thread flipper([&] {
            for (size_t k = 1; !stop; k++) pool.set_key(k % 3);
        });
        std::vector<std::thread> workers;
        for (int t = 0; t < 4; t++)
            workers.emplace_back([&] {
                for (int i = 0; i < 1000; i++) {
                    Lease<Fake> a(pool, make);
                    CHECK(a && a->alive && a->key < 3);
                    a.failed = i % 7 == 0;
                }
            });
        for (auto& w : workers) w.join();
        stop = true;
        flipper.join();
        CHECK(pool.idle() >= 1 && pool.idle() <= 4);
        g_pool = nullptr;
    }
    CHECK(g_made - made >= 1 && g_made - made == g_gone - gone);  // the pool took the rest with it
}

int main() {
    reuse_and_stale();
    failing_make();
    drains();
    threads();
    CHECK(g_made == g_gone);
    printf("pool ok: %ld workspaces made and destroyed, %ld drains\n", g_made.load(), g_drains.load());
    return 0;
}
