// Runtime of the lockstep shim (hip/hip_runtime.h beside this file says what it is for and what it cannot see).
// Header-only: one translation unit includes it.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <setjmp.h>
#include <ucontext.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define LS_ASAN 1
#include <sanitizer/common_interface_defs.h>
#endif
#endif

#define LS_SUBSETS 1             // this shim models declared subsets of a wave (ls::Subset, XM_IF_LANES of xm_kernels.hip)

extern "C" char __start_xm_lds[], __stop_xm_lds[];

namespace ls {

struct dim3 {
    uint32_t x, y, z;
    dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};

enum Op { OP_NONE, OP_BALLOT, OP_SHFL, OP_READLANE, OP_READFIRST, OP_DPP, OP_BPERM, OP_SETTLE, OP_SYNC, OP_ENTER, OP_LEAVE };
inline const char *op_name(int op)
{
    static const char *names[] = {"none", "__ballot", "__shfl_xor", "readlane", "readfirstlane", "update_dpp", "ds_bpermute",
                                  "lds_settle", "__syncthreads", "XM_IF_LANES", "the end of XM_IF_LANES"};
    return names[op];
}

constexpr int WAVE = 64;
constexpr int MAX_WAVES = 16;
constexpr size_t STACK_BYTES = 256 * 1024;
constexpr int WATCHDOG_SECONDS = 8;

struct Wave;
struct Lane {
    dim3 tid;
    Wave *wave;
    int id;                       // lane of the wave
    bool live;
    int op, line;                 // the rendezvous it waits at
    uint64_t dep;                 // what it brought there
    ucontext_t ctx;               // enters the lane; afterwards the switches are _setjmp / _longjmp, which make no system call
    jmp_buf jb;
    bool started;
    void *fake;                   // ASan's fake stack of this context while it is switched out
};

struct Wave {
    Lane lane[WAVE];
    int index;                    // wave of the workgroup
    int n_lanes;
    uint64_t snap[WAVE];          // the values of the rendezvous being resumed from
    bool snap_live[WAVE];
    // a declared subset (XM_IF_LANES): scope 0 = none, 1 = the lanes whose condition held run the marked statement,
    // 2 = the others run its else branch.  `active` lanes are scheduled; the others wait at the marker or at its end.
    int scope, scope_line;
    bool active[WAVE], member[WAVE], taken[WAVE];
    jmp_buf sched;
    const void *sched_bottom;
    size_t sched_size;
    std::atomic<int> at_op, at_line;                           // for the watchdog's message
};

inline thread_local Lane *cur = nullptr;
inline dim3 g_block, g_grid;
inline int g_fill = 0;
inline std::atomic<uint64_t> g_progress{0};
inline std::atomic<bool> g_running{false};
inline Wave *g_waves = nullptr;
inline int g_n_waves = 0;
inline char *g_stacks = nullptr;
inline const void *g_kernel = nullptr;                         // the std::function-free trampoline's argument
inline void (*g_invoke)(const void *) = nullptr;

inline void set_fill(int byte) { g_fill = byte; }

[[noreturn]] inline void die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
[[noreturn]] inline void die(const char *fmt, ...)
{
    char buf[600];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "lockstep: %s (workgroup %u,%u)\n", buf, g_block.x, g_block.y);
    fflush(stderr);
    _exit(3);
}

// ---- the workgroup barrier of the wave threads -------------------------------------------------------------------------
struct WgBarrier {
    std::mutex m;
    std::condition_variable cv;
    int expected = 0, waiting = 0;
    uint64_t gen = 0;
    void reset(int n) { expected = n; waiting = 0; }
    void arrive_and_wait(int wave, int line)
    {
        std::unique_lock<std::mutex> lk(m);
        if (++waiting == expected) { waiting = 0; ++gen; cv.notify_all(); return; }
        const uint64_t my = gen;
        if (!cv.wait_for(lk, std::chrono::seconds(WATCHDOG_SECONDS), [&] { return gen != my; }))
            die("watchdog: wave %d waits at __syncthreads of line %d, which the workgroup's other running waves never reach", wave, line);
    }
    void drop()                                                // a wave has ended: barriers no longer count it
    {
        std::lock_guard<std::mutex> lk(m);
        --expected;
        if (expected > 0 && waiting == expected) { waiting = 0; ++gen; cv.notify_all(); }
    }
};
inline WgBarrier g_barrier;

// ---- switching between a wave's scheduler and its lanes ----------------------------------------------------------------
inline void to_lane(Wave *w, Lane *l)
{
    cur = l;
#ifdef LS_ASAN
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, g_stacks + ((size_t)w->index * WAVE + l->id) * STACK_BYTES, STACK_BYTES);
#endif
    if (_setjmp(w->sched) == 0) {
        if (l->started) _longjmp(l->jb, 1);
        l->started = true;
        setcontext(&l->ctx);
    }
#ifdef LS_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
    cur = nullptr;
}

inline void to_sched(Lane *l, bool ended)
{
    Wave *w = l->wave;
#ifdef LS_ASAN
    __sanitizer_start_switch_fiber(ended ? nullptr : &l->fake, w->sched_bottom, w->sched_size);
#endif
    if (ended || _setjmp(l->jb) == 0) _longjmp(w->sched, 1);
#ifdef LS_ASAN
    __sanitizer_finish_switch_fiber(l->fake, &w->sched_bottom, &w->sched_size);
#endif
}

inline void lane_entry()
{
#ifdef LS_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &cur->wave->sched_bottom, &cur->wave->sched_size);
#endif
    g_invoke(g_kernel);
    Lane *l = cur;
    l->live = false;
    to_sched(l, true);
    abort();                                                   // an ended lane is never resumed
}

// a lane arrives at a cross-lane operation: leaves its value, runs again when all running lanes of the wave are there
inline void rendezvous(int op, int line, uint64_t value)
{
    Lane *l = cur;
    l->op = op;
    l->line = line;
    l->dep = value;
    to_sched(l, false);
}

inline void run_wave(Wave *w)
{
    for (int i = 0; i < w->n_lanes; ++i) {
        Lane *l = &w->lane[i];
        getcontext(&l->ctx);
        l->ctx.uc_stack.ss_sp = g_stacks + ((size_t)w->index * WAVE + i) * STACK_BYTES;
        l->ctx.uc_stack.ss_size = STACK_BYTES;
        l->ctx.uc_link = nullptr;
        makecontext(&l->ctx, lane_entry, 0);
        l->live = true;
        l->started = false;
        l->op = OP_NONE;
        l->fake = nullptr;
    }
    w->scope = 0;
    for (int i = 0; i < WAVE; ++i) w->active[i] = i < w->n_lanes;
    for (;;) {
        int first = -1;
        for (int i = 0; i < w->n_lanes; ++i) {
            Lane *l = &w->lane[i];
            if (!l->live || !w->active[i]) continue;
            to_lane(w, l);
            if (!l->live) continue;
            if (l->op == OP_LEAVE) {                           // done with its branch of a declared subset: waits for the others
                if (w->scope == 0 || l->line != w->scope_line)
                    die("wave %d: lane %d leaves the XM_IF_LANES of line %d, which the wave has not entered", w->index, i, l->line);
                w->active[i] = false;
                continue;
            }
            if (first < 0) first = i;
            else if (l->op != w->lane[first].op || l->line != w->lane[first].line)
                die("divergence in wave %d: lane %d is at %s of line %d, lane %d at %s of line %d", w->index, first,
                    op_name(w->lane[first].op), w->lane[first].line, i, op_name(l->op), l->line);
        }
        g_progress.fetch_add(1, std::memory_order_relaxed);
        if (first < 0) {
            if (w->scope == 1) {                               // the marked statement is done: now the else branch's lanes
                w->scope = 2;
                for (int i = 0; i < WAVE; ++i) w->active[i] = w->member[i] && !w->taken[i];
                continue;
            }
            if (w->scope == 2) {                               // everybody goes on together
                w->scope = 0;
                for (int i = 0; i < WAVE; ++i) w->active[i] = w->member[i];
                continue;
            }
            break;                                             // every lane has returned
        }
        const int op = w->lane[first].op, line = w->lane[first].line;
        for (int i = 0; i < WAVE; ++i) {
            const bool live = i < w->n_lanes && w->lane[i].live && w->active[i];
            w->snap_live[i] = live;
            w->snap[i] = live ? w->lane[i].dep : 0;
        }
        w->at_op = op;
        w->at_line = line;
        if (op == OP_ENTER) {
            if (w->scope != 0) die("wave %d: XM_IF_LANES of line %d inside the XM_IF_LANES of line %d: nested subsets are not modelled", w->index, line, w->scope_line);
            w->scope = 1;
            w->scope_line = line;
            for (int i = 0; i < WAVE; ++i) {
                w->member[i] = w->snap_live[i];
                w->taken[i] = w->snap_live[i] && (w->snap[i] & 1u) != 0u;
                w->active[i] = w->taken[i];
            }
        }
        if (op == OP_SYNC) {
            if (w->scope != 0) die("wave %d: __syncthreads of line %d inside the XM_IF_LANES of line %d", w->index, line, w->scope_line);
            g_barrier.arrive_and_wait(w->index, line);
        }
    }
    g_barrier.drop();
}

inline void watchdog()
{
    uint64_t seen = g_progress.load();
    int quiet = 0;
    for (;;) {
        std::this_thread::sleep_for(std::chrono::seconds(1));
        const uint64_t now = g_progress.load();
        if (!g_running.load() || now != seen) { seen = now; quiet = 0; continue; }
        if (++quiet < WATCHDOG_SECONDS) continue;
        char buf[400];
        int at = 0;
        for (int k = 0; k < g_n_waves && at < 340; ++k)
            at += snprintf(buf + at, sizeof buf - at, " wave %d after %s of line %d;", k, op_name(g_waves[k].at_op), g_waves[k].at_line.load());
        die("watchdog: no wave has reached a rendezvous or ended for %d s: a lane never arrives;%s", WATCHDOG_SECONDS, buf);
    }
}

inline void init_once()
{
    if (g_waves != nullptr) return;
    g_waves = new Wave[MAX_WAVES];
    g_stacks = (char *)mmap(nullptr, (size_t)MAX_WAVES * WAVE * STACK_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (g_stacks == (char *)MAP_FAILED) die("mmap of the lane stacks failed");
    std::thread(watchdog).detach();
}

template <typename F>
void launch(dim3 grid, dim3 block, const F &kernel)
{
    init_once();
    const uint32_t threads = block.x;
    if (block.y != 1 || block.z != 1 || threads == 0 || threads > MAX_WAVES * WAVE) die("block shape %u x %u x %u", block.x, block.y, block.z);
    g_grid = grid;
    g_kernel = &kernel;
    g_invoke = [](const void *k) { (*static_cast<const F *>(k))(); };
    g_n_waves = (int)((threads + WAVE - 1) / WAVE);
    for (uint32_t by = 0; by < grid.y; ++by)
        for (uint32_t bx = 0; bx < grid.x; ++bx) {
            g_block = dim3(bx, by, 0);
            memset(__start_xm_lds, g_fill, (size_t)(__stop_xm_lds - __start_xm_lds));
            g_barrier.reset(g_n_waves);
            for (int k = 0; k < g_n_waves; ++k) {
                Wave *w = &g_waves[k];
                w->index = k;
                w->n_lanes = (int)(threads - (uint32_t)k * WAVE < (uint32_t)WAVE ? threads - (uint32_t)k * WAVE : WAVE);
                w->at_op = OP_NONE;
                w->at_line = 0;
                for (int i = 0; i < w->n_lanes; ++i) {
                    w->lane[i].tid = dim3((uint32_t)(k * WAVE + i), 0, 0);
                    w->lane[i].wave = w;
                    w->lane[i].id = i;
                }
            }
            g_running = true;
            std::vector<std::thread> pool;
            for (int k = 1; k < g_n_waves; ++k) pool.emplace_back(run_wave, &g_waves[k]);
            run_wave(&g_waves[0]);
            for (auto &t : pool) t.join();
            g_running = false;
        }
}

// ---- the cross-lane operations ------------------------------------------------------------------------------------------
template <typename T>
inline uint64_t to_bits(T v)
{
    static_assert(sizeof(T) <= 8 && std::is_trivially_copyable<T>::value, "a lane's value is at most 64 bits");
    uint64_t b = 0;
    memcpy(&b, &v, sizeof(T));
    return b;
}
template <typename T>
inline T from_bits(uint64_t b)
{
    T v;
    memcpy(&v, &b, sizeof(T));
    return v;
}

inline uint64_t value_of(int lane, const char *what, int line)
{
    const Wave *w = cur->wave;
    if (lane < 0 || lane >= WAVE || !w->snap_live[lane])
        die("%s of line %d: lane %d reads lane %d, which is not running%s", what, line, cur->id, lane,
            w->scope != 0 ? " in this branch of XM_IF_LANES" : "");
    return w->snap[lane];
}

inline void syncthreads(int line) { rendezvous(OP_SYNC, line, 0); }
inline void settle(int line) { rendezvous(OP_SETTLE, line, 0); }

// XM_IF_LANES(cond): the lanes running together meet here with their cond; those with cond true then run the marked
// statement as a wave of their own (a ballot sees only them, reading another lane is an error, __syncthreads is one) until
// each has reached the statement's end or returned, then the others run the else branch the same way (run_wave)
struct Subset {
    bool taken;
    int line;
    Subset(bool cond, int line_) : taken(cond), line(line_) { rendezvous(OP_ENTER, line, cond ? 1u : 0u); }
    ~Subset() { rendezvous(OP_LEAVE, line, 0); }
    Subset(const Subset &) = delete;
};

inline uint64_t ballot(bool p, int line)
{
    rendezvous(OP_BALLOT, line, p ? 1u : 0u);
    const Wave *w = cur->wave;
    uint64_t m = 0;
    for (int i = 0; i < WAVE; ++i) m |= (w->snap[i] & 1u) << i;
    return m;
}

template <typename T>
inline T shfl_xor(T v, int mask, int width, int line)
{
    if (width != WAVE) die("__shfl_xor of line %d: width %d", line, width);
    rendezvous(OP_SHFL, line, to_bits(v));
    return from_bits<T>(value_of((cur->id ^ mask) & 63, "__shfl_xor", line));
}

inline int readlane(int v, int lane, int line)
{
    rendezvous(OP_READLANE, line, to_bits(v));
    return from_bits<int>(value_of(lane, "readlane", line));
}

inline int readfirstlane(int v, int line)
{
    rendezvous(OP_READFIRST, line, to_bits(v));
    const Wave *w = cur->wave;
    for (int i = 0; i < WAVE; ++i)
        if (w->snap_live[i]) return from_bits<int>(w->snap[i]);
    die("readfirstlane of line %d: no lane is running", line);
}

inline int ds_bpermute(int addr, int v, int line)
{
    rendezvous(OP_BPERM, line, to_bits(v));
    return from_bits<int>(value_of(((uint32_t)addr >> 2) & 63, "ds_bpermute", line));
}

// the DPP controls xm_kernels.hip uses, bound_ctrl off: a lane without a source, or in a row the row mask leaves out, keeps `old`
inline int update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl, int line)
{
    rendezvous(OP_DPP, line, to_bits(src));
    const Wave *w = cur->wave;
    const int lane = cur->id, row = lane >> 4, in_row = lane & 15;
    if (bank_mask != 0xf || bound_ctrl) die("update_dpp of line %d: bank mask 0x%x, bound_ctrl %d", line, bank_mask, (int)bound_ctrl);
    int from = -1;
    if ((ctrl == 0x111 || ctrl == 0x112 || ctrl == 0x114 || ctrl == 0x118) && row_mask == 0xf) {      // row_shr 1, 2, 4, 8
        const int by = ctrl & 15;
        from = in_row >= by ? lane - by : -1;
    } else if (ctrl == 0x142 && row_mask == 0xa) {                                                     // row_bcast15
        from = (row == 1 || row == 3) ? row * 16 - 1 : -1;
    } else if (ctrl == 0x143 && row_mask == 0xc) {                                                     // row_bcast31
        from = row >= 2 ? 31 : -1;
    } else if (ctrl == 0x138 && row_mask == 0xf) {                                                     // wave_shr 1
        from = lane - 1;
    } else {
        die("update_dpp of line %d: control 0x%x with row mask 0x%x is not modelled", line, ctrl, row_mask);
    }
    if (from >= 0 && w->scope != 0 && w->member[from] && w->lane[from].live && !w->snap_live[from])
        die("update_dpp of line %d: lane %d reads lane %d, which is not running in this branch of XM_IF_LANES", line, lane, from);
    if (from < 0 || !w->snap_live[from]) return old;
    return from_bits<int>(w->snap[from]);
}

inline uint32_t mbcnt_lo(uint32_t mask, uint32_t add)
{
    const int lane = cur->id;
    const uint32_t below = lane >= 32 ? 0xFFFFFFFFu : ((1u << lane) - 1u);
    return add + (uint32_t)__builtin_popcount(mask & below);
}
inline uint32_t mbcnt_hi(uint32_t mask, uint32_t add)
{
    const int lane = cur->id;
    const uint32_t below = lane <= 32 ? 0u : ((1u << (lane - 32)) - 1u);
    return add + (uint32_t)__builtin_popcount(mask & below);
}
inline uint32_t ubfe(uint32_t src, uint32_t off, uint32_t width)
{
    off &= 31u;
    width &= 31u;
    return width ? (src >> off) & ((1u << width) - 1u) : 0u;
}

}  // namespace ls
