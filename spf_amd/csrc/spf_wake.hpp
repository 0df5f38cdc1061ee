// spf_wake.hpp — the two protocols that put the pool's waiters to sleep and wake them (spf_pool.hpp, `struct Batch`).
//
// No HIP, nothing of the pool: futex words and the arithmetic that maps a slot to its word.  The pool's `wait`, `wait_value` and
// completion call what is here and hold no copy of it, so that tests/cpp/wake_protocol.cpp can run these very functions on the CPU
// and force the interleavings that the machine's own timing never produces.
//   * GroupTree  — by handle: waiters sleep in groups of eight and are woken as a tree;
//   * ChunkWords — host pointers: one word per 64 slots, woken chunk by chunk as the outputs arrive in pinned memory.
#pragma once

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <linux/futex.h>
#include <memory>
#include <sys/syscall.h>
#include <unistd.h>

// Test points.  The library is never built with SPF_WAKE_TEST; the test program defines it and supplies
// `void spf_wake_point(int tag, size_t index)`, in which it parks the calling thread where a scenario says so.
#ifdef SPF_WAKE_TEST
void spf_wake_point(int tag, size_t index);
#define SPF_WAKE_POINT(tag, index) spf_wake_point((tag), (index))
#else
#define SPF_WAKE_POINT(tag, index) ((void)0)
#endif

namespace spf_wake {

enum Point {
    kPointStore = 0, // wake_tree has just stored the word of group `index`
    kPointWake = 1,  // wake_tree has just come back from wake_group(`index`)
    kPointLook = 2,  // the waiter of slot `index` has looked at its word for the last time (and found it set)
};

inline void futex_wait(std::atomic<uint32_t>* w, uint32_t expected)
{
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0);
}
inline void futex_wake_all(std::atomic<uint32_t>* w)
{
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

// By handle the waiters are woken as a TREE: they sleep in groups of eight on a word per group; whoever completes the batch
// sets every word, wakes group 0, and every waiter that comes through wakes one child group (group g's member j: group
// 8 g + 1 + j) before it goes on.  One thread waking a thousand sleepers one by one took 6 us each (r06: 1.5 ms of a 256-caller
// batch's 5.8 ms cycle); the tree is three levels deep.  The completing thread also walks all groups in order and wakes what
// nobody has woken yet, so a waiter that never comes (an abandoned ticket) leaves no group asleep.
struct GroupTree {
    static constexpr size_t kTreeGroup = 8;
    std::unique_ptr<std::atomic<uint32_t>[]> gword, gwoken, gsleep; // [cap / 8 + 1]
    size_t n_final = 0; // slots of the batch: written by wake_tree ahead of the words, read only by who has seen a word set

    void init(size_t cap) // (throws std::bad_alloc)
    {
        const size_t ng = cap / kTreeGroup + 1;
        gword.reset(new std::atomic<uint32_t>[ng]);
        gwoken.reset(new std::atomic<uint32_t>[ng]);
        gsleep.reset(new std::atomic<uint32_t>[ng]);
        for (size_t g = 0; g < ng; g++) { gword[g].store(0); gwoken[g].store(0); gsleep[g].store(0); }
    }
    static size_t n_groups(size_t n) { return (n + kTreeGroup - 1) / kTreeGroup; }
    static size_t group_of(size_t slot) { return slot / kTreeGroup; }
    static size_t child_of(size_t slot) { return kTreeGroup * group_of(slot) + 1 + slot % kTreeGroup; } // (= slot + 1)
    bool is_set(size_t g) const { return gword[g].load(std::memory_order_acquire) != 0; }

    // a waiter announces itself in gsleep before it looks at the word for the last time; the waker sets the word before it looks at
    // gsleep (both sequentially consistent): a group nobody sleeps on costs no system call — operations pushed without a ticket have
    // no waiters at all, and a batch of 400 of them was 50 futex calls of ~2 us on the launcher's critical path
    void sleep_on_group(size_t g)
    {
        gsleep[g].fetch_add(1, std::memory_order_seq_cst);
        while (gword[g].load(std::memory_order_seq_cst) == 0) futex_wait(&gword[g], 0);
    }
    // Whoever calls this has seen a word at or below g set (its own, for a waiter; all of them, for the completing thread).  The
    // first caller is the only one that wakes, so the word of g MUST be set by then: sleepers woken with their word still 0 go
    // back to sleep, and every later wake_group(g) is skipped.  wake_tree's store order is what guarantees it.
    void wake_group(size_t g)
    {
        if (gwoken[g].exchange(1, std::memory_order_acq_rel) == 0 && gsleep[g].load(std::memory_order_seq_cst) != 0) futex_wake_all(&gword[g]);
    }
    // by the thread that completed the batch (n is final)
    void wake_tree(size_t n)
    {
        n_final = n;
        const size_t ng = n_groups(n);
        // INVARIANT: when a waiter can see word g, every word above g is already set — the words are stored from the highest
        // group down.  A waiter that finds its word set passes the wake on to a child group (child > g) at once, while this
        // loop may still be running (or its thread preempted); stored in ascending order, the child's sleepers were woken with
        // their word still 0, slept again, and the walk below skipped them because gwoken was already 1: asleep for good.
        for (size_t g = ng; g-- > 0;) {
            gword[g].store(1, std::memory_order_seq_cst);
            SPF_WAKE_POINT(kPointStore, g);
        }
        for (size_t g = 0; g < ng; g++) {
            wake_group(g);
            SPF_WAKE_POINT(kPointWake, g);
        }
    }
    // this waiter's share of the waking (it has seen its own word set, so n_final is there and every word above is set)
    void pass_on(size_t slot)
    {
        const size_t child = child_of(slot);
        if (child < n_groups(n_final)) wake_group(child);
    }
    // the waiter of a ticket: one per slot (the pool's spin loop, if any, comes first and looks at is_set)
    void wait_slot(size_t slot)
    {
        const size_t g = group_of(slot);
        if (!is_set(g)) sleep_on_group(g);
        SPF_WAKE_POINT(kPointLook, slot);
        pass_on(slot);
    }
    // whoever waits for a VALUE: any number of threads per slot, and none of them passes the wake on
    void wait_value(size_t slot)
    {
        const size_t g = group_of(slot);
        if (!is_set(g)) sleep_on_group(g);
    }
};

// The outputs of a host-pointer batch leave the GPU in up to kMaxChunks copies (each a multiple of kWordSlots slots, all but the
// last equal), each with its own event.  The waiters sleep on the word of their slot group (futex, 0 -> 1 when the group's bytes
// are in pinned memory or the batch failed): the callers of the first chunk copy out and come back while the later chunks are
// still crossing PCIe.  (Words per 64 slots rather than per chunk: a waiter may go to sleep before the batch is closed, when
// its size — and so the chunk boundaries — is not known yet.)
struct ChunkWords {
    static constexpr size_t kWordSlots = 64;
    static constexpr int kMaxWords = 64; // 4096 slots; the last word also takes whatever lies beyond
    static constexpr int kMaxChunks = 16;
    static int word_of(size_t slot) { return (int)std::min<size_t>(slot / kWordSlots, kMaxWords - 1); }
    std::atomic<uint32_t> chunk_word[kMaxWords] = {};
    size_t chunk_slots = 0; // slots per copy (set with n_chunks)
    int n_chunks = 0;       // set when the batch is enqueued

    // a batch of B slots (B > 0) in at most max_chunks copies
    void plan(size_t B, int max_chunks = kMaxChunks)
    {
        const size_t groups = (B + kWordSlots - 1) / kWordSlots;
        n_chunks = (int)std::min<size_t>(groups, (size_t)max_chunks);
        chunk_slots = (groups + n_chunks - 1) / n_chunks * kWordSlots;
        n_chunks = (int)((B + chunk_slots - 1) / chunk_slots);
    }
    void wait_slot(size_t slot)
    {
        std::atomic<uint32_t>& word = chunk_word[word_of(slot)];
        while (word.load(std::memory_order_acquire) == 0) futex_wait(&word, 0);
    }
    void wake_word(int w)
    {
        chunk_word[w].store(1, std::memory_order_release);
        futex_wake_all(&chunk_word[w]);
    }
    void wake_chunk(int i) // the words of copy i
    {
        // (the last word stands for every slot from 64 * (kMaxWords - 1) on, however many: only the last copy wakes it)
        const int w0 = word_of((size_t)i * chunk_slots);
        const int w1 = i + 1 < n_chunks ? std::min(word_of((size_t)(i + 1) * chunk_slots - 1), kMaxWords - 2) : kMaxWords - 1;
        for (int w = w0; w <= w1; w++)
            if (chunk_word[w].load(std::memory_order_relaxed) == 0) wake_word(w);
    }
    void wake_rest() // the last chunk — or, for a batch that failed, all of them
    {
        for (int w = 0; w < kMaxWords; w++)
            if (chunk_word[w].load(std::memory_order_relaxed) == 0) wake_word(w);
    }
};

} // namespace spf_wake
