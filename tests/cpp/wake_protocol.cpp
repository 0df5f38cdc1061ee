// wake_protocol.cpp — the pool's two sleeping protocols (spf_amd/csrc/spf_wake.hpp) under FORCED interleavings, on the CPU.
//
// The pool tests only ever see the timing the machine happens to produce; a lost wake-up needs a waiter to run inside a window
// of a few stores of the completing thread.  Here the completing thread is parked at a chosen test point of wake_tree
// (SPF_WAKE_POINT), a late waiter runs its whole path meanwhile, and every sleeper must still return.  Parts:
//   forced    every test point x every late slot whose child group exists, n in {9, 16, 17, 72, 73} exhaustively, a stated sample at
//             585 (three tree levels) and 4096 (512 groups); a sleeper parked in every group, eight in the group under test
//   variants  abandoned tickets (the parent of a group never comes), value-style sleepers (no pass-on, several per slot: one of
//             the two populations of every forced scenario), waiters that arrive when everything is set (they must not sleep)
//   chunks    ChunkWords::wake_chunk against a brute-force loop over the slots
//   stress    64 threads, random sizes and arrival delays, the three waiter kinds mixed: what ThreadSanitizer looks at
//   mutant    the ascending store order this header replaced, as a function of this file: the forced part must report it
// Nothing here may hang: a scenario waits at most 2 s for its sleepers (a cap, not a measurement: honest wake-ups take
// microseconds), then sets and wakes every word itself so that all threads end, prints the scenario, and the program exits 1.
//
// usage: wake_protocol            all parts; prints the counts, "mutant reported", "wake_protocol ok"
//        wake_protocol --mutant   the forced part with the mutant as the function under test: exits 1 and names the scenario
#define SPF_WAKE_TEST
#include "../../spf_amd/csrc/spf_wake.hpp"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <random>
#include <sched.h>
#include <string>
#include <thread>
#include <vector>

using namespace spf_wake;
using Clock = std::chrono::steady_clock;
using WakeTreeFn = void (*)(GroupTree&, size_t);

static constexpr auto kCap = std::chrono::seconds(2);    // per scenario, for the sleepers to return
static constexpr auto kSetup = std::chrono::seconds(20); // for threads to start and park (a loaded machine under TSan)

// The test's threads come from a pool that grows on demand: the parts below start some 80 000 short-lived threads between them,
// and creating each anew costs more than everything it does (under ThreadSanitizer about a millisecond apiece).
class Workers {
    struct Task { std::function<void()> fn; bool done = false; };
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<Task*> queue;
    std::vector<std::thread> threads;
    size_t idle = 0;
    bool stop = false;
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            idle++;
            cv_work.wait(lk, [&] { return stop || !queue.empty(); });
            idle--;
            if (queue.empty()) return;
            Task* t = queue.front();
            queue.pop_front();
            lk.unlock();
            t->fn();
            lk.lock();
            t->done = true;
            cv_done.notify_all();
        }
    }

public:
    using Handle = Task*;
    Handle start(std::function<void()> fn)
    {
        Task* t = new Task{std::move(fn)};
        std::lock_guard<std::mutex> g(mu);
        queue.push_back(t);
        if (queue.size() > idle) threads.emplace_back([this] { loop(); });
        else cv_work.notify_one();
        return t;
    }
    void finish(Handle t)
    {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&] { return t->done; });
        }
        delete t;
    }
    void shutdown()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
            cv_work.notify_all();
        }
        for (auto& x : threads) x.join();
        threads.clear();
    }
};
static Workers g_workers;
struct Job { // (what std::thread would be: starts at once, has to be joined)
    Workers::Handle h = nullptr;
    Job() = default;
    template <class F> explicit Job(F&& f) : h(g_workers.start(std::forward<F>(f))) {}
    Job(Job&& o) noexcept : h(o.h) { o.h = nullptr; }
    Job& operator=(Job&& o) noexcept { h = o.h; o.h = nullptr; return *this; }
    bool joinable() const { return h != nullptr; }
    void join() { g_workers.finish(h); h = nullptr; }
};
// (timed waits against the system clock: the form of the condition variable's wait that ThreadSanitizer knows about)
template <class Pred> static bool wait_capped(std::condition_variable& cv, std::unique_lock<std::mutex>& lk, Clock::duration cap, Pred pred)
{
    return cv.wait_until(lk, std::chrono::system_clock::now() + cap, pred);
}

static void wake_tree_fixed(GroupTree& t, size_t n) { t.wake_tree(n); }
// THE MUTANT: wake_tree as it was, the words stored from group 0 up.  A waiter that sees word g may then wake a child whose
// word is still 0.
static void wake_tree_ascending(GroupTree& t, size_t n)
{
    t.n_final = n;
    const size_t ng = GroupTree::n_groups(n);
    for (size_t g = 0; g < ng; g++) {
        t.gword[g].store(1, std::memory_order_seq_cst);
        SPF_WAKE_POINT(kPointStore, g);
    }
    for (size_t g = 0; g < ng; g++) {
        t.wake_group(g);
        SPF_WAKE_POINT(kPointWake, g);
    }
}

// ---- the test points: the completing thread parks at one of them, the late waiter (optionally) behind its last look
enum Role { kNobody = 0, kCompleter, kLate };
struct Hook {
    int stop_tag = -1;
    size_t stop_index = 0;
    bool hold_look = false;
    std::mutex mu;
    std::condition_variable cv;
    bool paused = false, resume = false, at_look = false, look_resume = false;
    void release_all()
    {
        std::lock_guard<std::mutex> g(mu);
        resume = look_resume = true;
        cv.notify_all();
    }
};
static thread_local Hook* tl_hook = nullptr;
static thread_local Role tl_role = kNobody;
void spf_wake_point(int tag, size_t index)
{
    Hook* h = tl_hook;
    if (!h) return;
    if (tl_role == kCompleter && tag == h->stop_tag && index == h->stop_index) {
        std::unique_lock<std::mutex> lk(h->mu);
        h->paused = true;
        h->cv.notify_all();
        h->cv.wait(lk, [&] { return h->resume; });
    } else if (tl_role == kLate && tag == kPointLook && h->hold_look) {
        std::unique_lock<std::mutex> lk(h->mu);
        h->at_look = true;
        h->cv.notify_all();
        h->cv.wait(lk, [&] { return h->look_resume; });
    }
}

// ---- a population of sleepers on one tree
struct Sleeper {
    size_t slot = 0;
    bool by_value = false;
    std::atomic<int> returned{0}, tid{0};
    Clock::time_point t_ret;
};
// the scheduler's word on a thread: 'S' once it is blocked inside its futex call ('R' from the moment a futex wake reaches it)
static char thread_state(int tid)
{
    char path[64], buf[512];
    snprintf(path, sizeof path, "/proc/self/task/%d/stat", tid);
    FILE* f = fopen(path, "r");
    if (!f) return '?';
    const size_t k = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[k] = 0;
    const char* p = strrchr(buf, ')');
    return p && p[1] == ' ' ? p[2] : '?';
}
struct Crowd {
    GroupTree& t;
    std::vector<std::unique_ptr<Sleeper>> who;
    std::vector<Job> th;
    std::vector<uint32_t> expect; // sleepers per group
    std::mutex mu;
    std::condition_variable cv;
    size_t n_returned = 0;
    explicit Crowd(GroupTree& tree, size_t ng) : t(tree), expect(ng, 0) {}
    void add(size_t slot, bool by_value)
    {
        who.emplace_back(new Sleeper);
        who.back()->slot = slot;
        who.back()->by_value = by_value;
        expect[GroupTree::group_of(slot)]++;
    }
    void done(Sleeper* s)
    {
        s->t_ret = Clock::now();
        s->returned.store(1, std::memory_order_release);
        std::lock_guard<std::mutex> g(mu);
        n_returned++;
        cv.notify_all();
    }
    void start()
    {
        for (auto& s : who)
            th.emplace_back([this, p = s.get()] {
                p->tid.store((int)syscall(SYS_gettid), std::memory_order_release);
                if (p->by_value) t.wait_value(p->slot);
                else t.wait_slot(p->slot);
                done(p);
            });
    }
    // parked: every sleeper has announced itself in gsleep (what the protocol itself goes by)
    bool wait_parked()
    {
        const auto until = Clock::now() + kSetup;
        for (size_t g = 0; g < expect.size(); g++)
            while (t.gsleep[g].load(std::memory_order_seq_cst) != expect[g]) {
                if (Clock::now() > until) return false;
                (void)sched_yield();
            }
        return true;
    }
    // ... and, for one group, the scheduler agrees: each sleeper that has not returned is blocked in the kernel.  gsleep says that
    // a sleeper WILL wait; a scenario that counts on sleepers having been woken for nothing and gone back to sleep needs to know
    // that they ARE back (a woken thread that has not run yet would find the word the completing thread sets next).
    bool wait_blocked(long group)
    {
        const auto until = Clock::now() + kSetup;
        for (auto& s : who) {
            if ((long)GroupTree::group_of(s->slot) != group) continue;
            while (!s->returned.load(std::memory_order_acquire) && (s->tid.load(std::memory_order_acquire) == 0 || thread_state(s->tid.load()) != 'S')) {
                if (Clock::now() > until) return false;
                (void)sched_yield();
            }
        }
        return true;
    }
    bool wait_returned(size_t extra, Clock::duration cap)
    {
        std::unique_lock<std::mutex> lk(mu);
        return wait_capped(cv, lk, cap, [&] { return n_returned == who.size() + extra; });
    }
    void rescue(size_t ng) // set and wake every word: all threads end
    {
        for (size_t g = 0; g < ng; g++) {
            t.gword[g].store(1, std::memory_order_seq_cst);
            futex_wake_all(&t.gword[g]);
        }
    }
    void join()
    {
        for (auto& x : th) x.join();
    }
};

struct Scenario {
    size_t n = 0;
    int stop_tag = -1; // kPointStore / kPointWake, -1: the completing thread runs through
    size_t stop_index = 0;
    long late_slot = -1;  // the waiter that arrives while the completing thread is parked
    bool hold_look = false; // ... and stays behind its last look until the completing thread has finished
    bool values = false;  // group under test: eight value-style sleepers on ONE slot (else: its tickets, filled up with values)
    long abandoned = -1;  // full population of ticket waiters, but nobody for this slot: its child group is the one under test
};
static std::string name_of(const Scenario& s)
{
    char buf[200];
    const char* tag = s.stop_tag == kPointStore ? "store" : s.stop_tag == kPointWake ? "wake" : "none";
    snprintf(buf, sizeof buf, "n=%zu stop=%s[%zu] late_slot=%ld hold_look=%d group_under_test=%ld sleepers=%s abandoned_slot=%ld", s.n, tag,
             s.stop_index, s.late_slot, (int)s.hold_look, s.late_slot >= 0 ? s.late_slot + 1 : s.abandoned + 1, s.values ? "values" : "tickets", s.abandoned);
    return buf;
}
struct Outcome {
    bool ok = false;
    std::string why;
    size_t stuck = 0, stuck_under_test = 0, under_test = 0;
};
static double g_max_latency_us = 0;

static Outcome run_scenario(const Scenario& sc, WakeTreeFn fn)
{
    Outcome out;
    const size_t n = sc.n, ng = GroupTree::n_groups(n);
    GroupTree t;
    t.init(n);
    Crowd crowd(t, ng);
    const long target = sc.late_slot >= 0 ? sc.late_slot + 1 : (sc.abandoned >= 0 ? sc.abandoned + 1 : -1); // (child_of(slot) = slot + 1)
    for (size_t g = 0; g < ng; g++) {
        const size_t lo = GroupTree::kTreeGroup * g, hi = std::min(n, lo + GroupTree::kTreeGroup);
        if ((long)g == target) {
            size_t k = 0;
            if (!sc.values)
                for (size_t s = lo; s < hi; s++, k++) crowd.add(s, false);
            for (; k < 8; k++) crowd.add(lo, true);
        } else if (sc.abandoned >= 0) {
            for (size_t s = lo; s < hi; s++)
                if ((long)s != sc.abandoned) crowd.add(s, false);
        } else {
            for (size_t s = lo; s < hi; s++)
                if ((long)s != sc.late_slot) { crowd.add(s, false); break; }
        }
    }
    for (auto& s : crowd.who) out.under_test += (long)GroupTree::group_of(s->slot) == target;
    Hook hook;
    hook.stop_tag = sc.stop_tag;
    hook.stop_index = sc.stop_index;
    hook.hold_look = sc.hold_look;
    std::atomic<int> completer_done{0}, late_done{0};
    Job completer, late;
    auto fail_setup = [&](const char* why) {
        hook.release_all();
        crowd.rescue(ng);
        if (completer.joinable()) completer.join();
        if (late.joinable()) late.join();
        crowd.join();
        out.why = why;
        return out;
    };
    crowd.start();
    if (!crowd.wait_parked() || !crowd.wait_blocked(target)) return fail_setup("setup: the sleepers did not park");
    Clock::time_point t_go = Clock::now();
    completer = Job([&] {
        tl_hook = &hook;
        tl_role = kCompleter;
        fn(t, n);
        tl_hook = nullptr;
        completer_done.store(1, std::memory_order_release);
    });
    size_t extra = 0;
    if (sc.stop_tag >= 0) {
        {
            std::unique_lock<std::mutex> lk(hook.mu);
            if (!wait_capped(hook.cv, lk, kSetup, [&] { return hook.paused; })) {
                lk.unlock();
                return fail_setup("setup: the completing thread never reached its test point");
            }
        }
        if (sc.late_slot >= 0) {
            extra = 1;
            const size_t gl = GroupTree::group_of((size_t)sc.late_slot);
            late = Job([&] {
                tl_hook = &hook;
                tl_role = kLate;
                t.wait_slot((size_t)sc.late_slot);
                tl_hook = nullptr;
                late_done.store(1, std::memory_order_release);
                std::lock_guard<std::mutex> g(crowd.mu);
                crowd.n_returned++;
                crowd.cv.notify_all();
            });
            // the late waiter runs its whole path: until it is through, asleep (announced in gsleep), or held behind its last look
            const auto until = Clock::now() + kSetup;
            for (;;) {
                if (late_done.load(std::memory_order_acquire)) break;
                if (t.gsleep[gl].load(std::memory_order_seq_cst) == crowd.expect[gl] + 1) break;
                {
                    std::lock_guard<std::mutex> g(hook.mu);
                    if (hook.at_look) break;
                }
                if (Clock::now() > until) return fail_setup("setup: the late waiter neither finished nor slept");
                (void)sched_yield();
            }
            // whatever the late waiter woke in the group under test has run and settled: back asleep, or gone
            if (!crowd.wait_blocked(target)) return fail_setup("setup: the group under test did not settle");
        }
        t_go = Clock::now();
        {
            std::lock_guard<std::mutex> g(hook.mu);
            hook.resume = true;
            hook.cv.notify_all();
        }
        if (sc.hold_look) {
            const auto until = Clock::now() + kSetup;
            while (!completer_done.load(std::memory_order_acquire)) {
                if (Clock::now() > until) return fail_setup("setup: the completing thread did not finish");
                (void)sched_yield();
            }
            std::lock_guard<std::mutex> g(hook.mu);
            hook.look_resume = true;
            hook.cv.notify_all();
        }
    }
    out.ok = crowd.wait_returned(extra, kCap);
    if (!out.ok) {
        for (auto& s : crowd.who)
            if (!s->returned.load(std::memory_order_acquire)) {
                out.stuck++;
                out.stuck_under_test += (long)GroupTree::group_of(s->slot) == target;
            }
        if (extra && !late_done.load(std::memory_order_acquire)) out.stuck++;
        out.why = "sleepers still asleep after 2 s";
        hook.release_all();
        crowd.rescue(ng);
    }
    completer.join();
    if (late.joinable()) late.join();
    crowd.join();
    if (out.ok)
        for (auto& s : crowd.who)
            g_max_latency_us = std::max(g_max_latency_us, std::chrono::duration<double, std::micro>(s->t_ret - t_go).count());
    return out;
}

static int report(const char* part, const Scenario& sc, const Outcome& o)
{
    printf("FAILED %s: %s: %s: %zu sleepers stuck, %zu of %zu in the group under test\n", part, name_of(sc).c_str(), o.why.c_str(), o.stuck, o.stuck_under_test, o.under_test);
    fflush(stdout);
    return 1;
}

// ---- forced interleavings
static void add_all_points(std::vector<Scenario>& v, size_t n, long late, bool hold, bool values)
{
    const size_t ng = GroupTree::n_groups(n);
    for (int tag : {(int)kPointStore, (int)kPointWake})
        for (size_t i = 0; i < ng; i++) {
            Scenario s;
            s.n = n; s.stop_tag = tag; s.stop_index = i; s.late_slot = late; s.hold_look = hold; s.values = values;
            v.push_back(s);
        }
}
static std::vector<Scenario> exhaustive_scenarios()
{
    std::vector<Scenario> v;
    for (size_t n : {9, 16, 17, 72, 73}) {
        const size_t ng = GroupTree::n_groups(n);
        for (size_t late = 0; late + 1 < ng; late++) // every late slot whose child group (late + 1) exists
            for (int hold = 0; hold < 2; hold++)
                for (int values = 0; values < 2; values++) add_all_points(v, n, (long)late, hold != 0, values != 0);
    }
    return v;
}
// THE SAMPLE at 585 and 4096.  Late slots: the first and last member of group 0 (children 1 and 8), the first member of group 1
// (child 9, the first group of the next level), slot 71 (child 72, the last group of that level), at 4096 also 72 (child 73, the
// first group of the deepest level) and 300 (in its middle), and the parent of the LAST group (72 at 585, 510 at 4096).  Test
// points, for late slot s in group g with child c = s + 1: behind the first store, the stores of c, g and 0, and behind the wakes
// of 0, g, c and the last group.  Tickets / run-through and values / held-behind-the-look alternate.
static std::vector<Scenario> sampled_scenarios()
{
    std::vector<Scenario> v;
    for (size_t n : {585, 4096}) {
        const size_t ng = GroupTree::n_groups(n);
        std::vector<size_t> lates = {0, 7, 8, 71};
        if (n == 4096) { lates.push_back(72); lates.push_back(300); }
        lates.push_back(ng - 2);
        for (size_t late : lates) {
            const size_t g = GroupTree::group_of(late), c = late + 1;
            std::vector<std::pair<int, size_t>> pts = {{kPointStore, ng - 1}, {kPointStore, c}, {kPointStore, g}, {kPointStore, 0},
                                                       {kPointWake, 0}, {kPointWake, g}, {kPointWake, c}, {kPointWake, ng - 1}};
            for (size_t i = 0; i < pts.size(); i++) {
                bool seen = false;
                for (size_t j = 0; j < i; j++) seen = seen || pts[j] == pts[i];
                if (seen) continue;
                Scenario s;
                s.n = n; s.stop_tag = pts[i].first; s.stop_index = pts[i].second; s.late_slot = (long)late;
                s.values = s.hold_look = (v.size() & 1) != 0;
                v.push_back(s);
            }
        }
    }
    return v;
}
static Scenario named_scenario() // the one the defect was found in: eight sleepers on group 1, the completer parked behind gword[0] = 1
{
    Scenario s;
    s.n = 72; s.stop_tag = kPointStore; s.stop_index = 0; s.late_slot = 0;
    return s;
}

static int run_forced(WakeTreeFn fn)
{
    const auto ex = exhaustive_scenarios(), sa = sampled_scenarios();
    for (const auto* list : {&ex, &sa})
        for (const Scenario& sc : *list) {
            const Outcome o = run_scenario(sc, fn);
            if (!o.ok) return report("forced", sc, o);
        }
    printf("forced: %zu exhaustive + %zu sampled scenarios, 0 failed\n", ex.size(), sa.size());
    return 0;
}

// ---- variants
static int run_variants()
{
    size_t n_abandoned = 0, n_late = 0;
    // abandoned tickets: everybody waits but the parent of one group; the completing thread's walk has to wake that group.
    // Run through, and with the completing thread parked behind its wake of group 0 (the waiters start passing the wake on
    // while the walk stands still).
    for (size_t n : {9, 16, 17, 72, 73, 585}) {
        const size_t ng = GroupTree::n_groups(n);
        std::vector<size_t> parents;
        if (n <= 73) for (size_t p = 0; p + 1 < ng; p++) parents.push_back(p);
        else parents = {0, 7, 8, 71, 72};
        for (size_t p : parents)
            for (int stop = 0; stop < 2; stop++) {
                Scenario s;
                s.n = n; s.abandoned = (long)p;
                if (stop) { s.stop_tag = kPointWake; s.stop_index = 0; }
                const Outcome o = run_scenario(s, wake_tree_fixed);
                if (!o.ok) return report("abandoned", s, o);
                n_abandoned++;
            }
    }
    // nobody waits at all below the leaves: value-style sleepers only, eight on one slot of every group
    for (size_t n : {9, 73, 585}) {
        const size_t ng = GroupTree::n_groups(n);
        GroupTree t;
        t.init(n);
        Crowd crowd(t, ng);
        for (size_t g = 0; g < ng; g++)
            for (int k = 0; k < 8; k++) crowd.add(std::min(n - 1, 8 * g + 3), true);
        crowd.start();
        bool ok = crowd.wait_parked();
        if (ok) {
            t.wake_tree(n);
            ok = crowd.wait_returned(0, kCap);
        }
        if (!ok) crowd.rescue(ng);
        crowd.join();
        if (!ok) {
            printf("FAILED values only: n=%zu: eight value-style sleepers per group, no ticket waiters: not all returned\n", n);
            return 1;
        }
        n_abandoned++;
    }
    // waiters that arrive after everything is set: they return, and none of them announces itself as a sleeper
    for (size_t n : {1, 8, 9, 16, 17, 72, 73, 585, 4096}) {
        const size_t ng = GroupTree::n_groups(n);
        GroupTree t;
        t.init(n);
        t.wake_tree(n);
        std::atomic<int> through{0};
        std::mutex mu;
        std::condition_variable cv;
        Job th([&] {
            for (size_t s = 0; s < n; s++) {
                t.wait_slot(s);
                t.wait_value(s);
                t.wait_value(s);
            }
            std::lock_guard<std::mutex> g(mu);
            through.store(1);
            cv.notify_all();
        });
        bool ok;
        {
            std::unique_lock<std::mutex> lk(mu);
            ok = wait_capped(cv, lk, kCap, [&] { return through.load() != 0; });
        }
        if (!ok)
            for (size_t g = 0; g < ng; g++) futex_wake_all(&t.gword[g]);
        th.join();
        for (size_t g = 0; g < ng; g++) ok = ok && t.gsleep[g].load() == 0 && t.gword[g].load() == 1;
        if (!ok) {
            printf("FAILED late arrivals: n=%zu: a waiter that found everything set slept, or a word was left unset\n", n);
            return 1;
        }
        n_late++;
    }
    printf("variants: %zu abandoned or value-only + %zu late-arrival scenarios, 0 failed\n", n_abandoned, n_late);
    return 0;
}

// ---- chunk words against a plain statement
// After wake_chunk(0..i): a word that holds a slot below n is set if and only if every slot of it below n lies in a chunk <= i
// (slot s lies in chunk s / chunk_slots); a word is never set while a slot of it is still to come; after the last chunk every
// word is set, the ones no slot maps to included (only the last chunk sets those: nobody can wait there).
static int check_chunks(size_t n, size_t chunk_slots, int n_chunks, const char* how)
{
    ChunkWords cw;
    cw.chunk_slots = chunk_slots;
    cw.n_chunks = n_chunks;
    for (int i = 0; i < n_chunks; i++) {
        cw.wake_chunk(i);
        bool has[ChunkWords::kMaxWords] = {}, all_in[ChunkWords::kMaxWords];
        for (bool& b : all_in) b = true;
        for (size_t s = 0; s < n; s++) { // the reference: slot by slot
            const size_t w = std::min<size_t>(s / 64, 63);
            has[w] = true;
            if (s / chunk_slots > (size_t)i) all_in[w] = false;
        }
        for (int w = 0; w < ChunkWords::kMaxWords; w++) {
            const bool set = cw.chunk_word[w].load() != 0;
            const bool bad = has[w] ? set != all_in[w] : (i + 1 == n_chunks && !set);
            if (bad) {
                printf("FAILED chunks (%s): n=%zu chunk_slots=%zu n_chunks=%d: after chunk %d word %d is %s\n", how, n, chunk_slots, n_chunks, i, w, set ? "set" : "not set");
                return 1;
            }
        }
    }
    return 0;
}
static int run_chunks()
{
    size_t plans = 0, sleeper_runs = 0;
    for (size_t n : {1, 63, 64, 65, 4095, 4096, 4097, 10000}) {
        for (int m = 1; m <= 16; m++) {
            // as the pool plans a batch of n with at most m copies ...
            ChunkWords p;
            p.plan(n, m);
            if (p.chunk_slots % 64 != 0 || p.n_chunks < 1 || p.n_chunks > m || (size_t)p.n_chunks * p.chunk_slots < n || (size_t)(p.n_chunks - 1) * p.chunk_slots >= n) {
                printf("FAILED chunks: plan(%zu, %d) gives chunk_slots=%zu n_chunks=%d\n", n, m, p.chunk_slots, p.n_chunks);
                return 1;
            }
            if (check_chunks(n, p.chunk_slots, p.n_chunks, "plan")) return 1;
            plans++;
            // ... and every other multiple of 64 that cuts n into exactly m copies
            for (size_t cs = 64; cs <= n + 63; cs += 64)
                if ((n + cs - 1) / cs == (size_t)m && cs != p.chunk_slots) {
                    if (check_chunks(n, cs, m, "every multiple of 64")) return 1;
                    plans++;
                }
        }
        // sleepers on the first, a middle and the last word, the copies arriving one by one
        ChunkWords cw;
        cw.plan(n);
        const size_t slots[3] = {0, n / 2, n - 1};
        std::atomic<int> through_chunk{-1};
        std::atomic<int> early{0};
        std::mutex mu;
        std::condition_variable cv;
        int n_back = 0;
        std::vector<Job> th;
        for (int k = 0; k < 3; k++)
            for (int rep = 0; rep < 2; rep++)
                th.emplace_back([&, s = slots[k]] {
                    cw.wait_slot(s);
                    if (through_chunk.load() < (int)(s / cw.chunk_slots)) early.fetch_add(1); // woken before its copy was announced
                    std::lock_guard<std::mutex> g(mu);
                    n_back++;
                    cv.notify_all();
                });
        for (int i = 0; i < cw.n_chunks; i++) {
            for (int y = 0; y < 50; y++) (void)sched_yield(); // (lets the sleepers reach their futex: not needed for the assertion)
            through_chunk.store(i);
            cw.wake_chunk(i);
        }
        bool ok;
        {
            std::unique_lock<std::mutex> lk(mu);
            ok = wait_capped(cv, lk, kCap, [&] { return n_back == 6; });
        }
        if (!ok) cw.wake_rest();
        for (auto& x : th) x.join();
        if (!ok || early.load()) {
            printf("FAILED chunks: n=%zu: sleepers on slots 0, %zu, %zu: %s\n", n, n / 2, n - 1, ok ? "one returned before its chunk" : "not all returned");
            return 1;
        }
        sleeper_runs++;
    }
    printf("chunks: %zu plans against the slot loop + %zu sleeper runs, 0 failed\n", plans, sleeper_runs);
    return 0;
}

// ---- randomised stress: for ThreadSanitizer
static int run_stress()
{
    constexpr int kThreads = 64, kRounds = 300;
    std::mt19937_64 rng(20261015);
    auto spin_for = [](unsigned us) {
        const auto until = Clock::now() + std::chrono::microseconds(us);
        while (Clock::now() < until) __builtin_ia32_pause();
    };
    for (int round = 0; round < kRounds; round++) {
        const size_t n = 1 + rng() % 600, ng = GroupTree::n_groups(n);
        GroupTree t;
        t.init(n);
        ChunkWords cw;
        cw.plan(n);
        std::vector<size_t> perm(n);
        for (size_t i = 0; i < n; i++) perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        struct W { int kind; size_t slot; unsigned delay; };
        std::vector<W> w(kThreads);
        size_t tickets = 0;
        for (auto& x : w) {
            x.kind = (int)(rng() % 3); // 0: ticket (one per slot), 1: value, 2: host-pointer chunk word
            if (x.kind == 0 && tickets == n) x.kind = 1;
            x.slot = x.kind == 0 ? perm[tickets++] : rng() % n;
            x.delay = (unsigned)(rng() % 150);
        }
        const unsigned completer_delay = (unsigned)(rng() % 150);
        std::mutex mu;
        std::condition_variable cv;
        int n_back = 0;
        std::vector<Job> th;
        for (const W& x : w)
            th.emplace_back([&, x] {
                spin_for(x.delay);
                if (x.kind == 0) t.wait_slot(x.slot);
                else if (x.kind == 1) t.wait_value(x.slot);
                else cw.wait_slot(x.slot);
                std::lock_guard<std::mutex> g(mu);
                n_back++;
                cv.notify_all();
            });
        Job completer([&] {
            spin_for(completer_delay);
            t.wake_tree(n);
            for (int i = 0; i + 1 < cw.n_chunks; i++) cw.wake_chunk(i);
            cw.wake_rest();
        });
        bool ok;
        {
            std::unique_lock<std::mutex> lk(mu);
            ok = wait_capped(cv, lk, kCap, [&] { return n_back == kThreads; });
        }
        completer.join();
        if (!ok) {
            for (size_t g = 0; g < ng; g++) { t.gword[g].store(1); futex_wake_all(&t.gword[g]); }
            cw.wake_rest();
        }
        for (auto& x : th) x.join();
        if (!ok) {
            printf("FAILED stress: round %d, n=%zu: %d of %d threads returned within 2 s\n", round, n, n_back, kThreads);
            return 1;
        }
    }
    printf("stress: %d rounds of %d threads, 0 failed\n", kRounds, kThreads);
    return 0;
}

static int run_all(int argc, char** argv)
{
    if (argc > 1 && strcmp(argv[1], "--mutant") == 0) {
        // the named scenario first (so that it is the one reported), then the whole forced part
        const Scenario sc = named_scenario();
        const Outcome o = run_scenario(sc, wake_tree_ascending);
        if (!o.ok) return report("forced (mutant: ascending stores)", sc, o);
        return run_forced(wake_tree_ascending) ? 1 : (printf("the mutant passed the forced part\n"), 0);
    }
    if (run_forced(wake_tree_fixed)) return 1;
    if (run_variants()) return 1;
    if (run_chunks()) return 1;
    if (run_stress()) return 1;
    // the conditions bite: the same scenario runner, the ascending store order
    {
        const double keep = g_max_latency_us;
        const Scenario sc = named_scenario();
        const Outcome o = run_scenario(sc, wake_tree_ascending);
        g_max_latency_us = keep;
        if (o.ok || o.why.rfind("setup", 0) == 0) {
            printf("FAILED mutant: ascending stores went unnoticed in %s (%s)\n", name_of(sc).c_str(), o.ok ? "every sleeper returned" : o.why.c_str());
            return 1;
        }
        printf("mutant reported: ascending stores, %s: %zu of %zu sleepers of group 1 still asleep after 2 s\n", name_of(sc).c_str(), o.stuck_under_test, o.under_test);
    }
    printf("largest wake latency: %.0f us (completing thread released -> last sleeper back, over the forced and abandoned scenarios)\n", g_max_latency_us);
    printf("wake_protocol ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int rc = run_all(argc, argv);
    g_workers.shutdown();
    return rc;
}
