// Stand-in for <hip/hip_runtime.h>: with this directory first on the include path and XM_LOCKSTEP_HOST defined,
// xenomapper_amd/csrc/xm_kernels.hip compiles as plain C++ (ROCm's host clang++, -x c++) and its kernels execute on the CPU,
// lane by lane, where ASan and UBSan can watch them (tests/lockstep_place_host.cpp, tests/test_lockstep_place_cpu.py: the fused
// step's launches; tests/lockstep_kernels_host.cpp, tests/test_lockstep_kernels_cpu.py: every other launcher of the file).
//
// How a launch executes (lockstep.h has the runtime):
//   - workgroups run one after another; the waves of a workgroup run concurrently, one host thread each;
//   - the 64 lanes of a wave are 64 contexts of that thread, each with a stack of its own.  A lane runs until it reaches a
//     cross-lane operation or ends; when every lane of the wave that is still running has arrived, the operation is
//     evaluated and all of them go on.  (One host thread per lane would do the same, but a rendezvous of 64 threads is 64
//     trips through the kernel's scheduler and the scatter makes some 300 of them per granule; switching contexts inside
//     one thread costs a _setjmp / _longjmp pair per lane and makes the order of the lanes repeatable: lane 0 first.)
//   - every rendezvous carries its kind and its source line.  Lanes that meet at different lines or in different
//     operations end the program with a message naming both lines; a wave that makes no progress for some seconds (a lane in
//     an endless loop, a wave waiting at a barrier the others never reach) ends it through the watchdog.  Lanes that have
//     returned take no part: a ballot sees them as 0, reading one of them is an error;
//   - a cross-lane operation that only part of the running lanes reach is therefore an error -- also where HIP allows it (a
//     ballot inside a divergent branch is a ballot over the lanes in that branch) -- unless the kernel source declares the
//     subset: `XM_IF_LANES(cond) statement [else statement]` (xm_kernels.hip; a plain `if` on the device).  All lanes running
//     together meet at the marker with their cond.  Those with cond true run the statement as a wave of their own until each
//     has reached its end or returned: a ballot sees them only (the other lanes' bits are 0), __shfl_xor, readlane,
//     ds_bpermute and update_dpp from a lane outside the subset end the program as reading a returned lane does, and so
//     does a __syncthreads inside the statement.  Then the lanes with cond false run the else branch the same way, and
//     everybody goes on together.  A marker inside a marked statement ends the program: nothing needs it yet.  The rule for
//     unmarked code is as strict as before.  lockstep.h defines LS_SUBSETS to say that it models this: xm_kernels.hip opens the
//     scope only then, so it still compiles against a shim that does not;
//   - __shared__ is a static in the section xm_lds: one copy serves the workgroup.  The runtime fills the section
//     from __start_xm_lds to __stop_xm_lds with the byte of ls::set_fill() before every workgroup, so that a kernel which
//     reads LDS it has not written gives results that depend on the fill.  ASan puts no redzones between globals of a
//     named section: a store past one LDS array into the next is NOT reported, it shows only through wrong results;
//   - lds_settle() is a wave rendezvous: on the host that is what it means, this wave's LDS operations are done;
//   - atomicAdd / atomicOr are host atomics, __syncthreads a barrier of the workgroup's wave threads.
//
// What it cannot see: timing between workgroups, the memory model of the device, alignment traps, anything outside the
// launches it is given.
//
// False alarms: code that relies on lockstep between one lane's LDS write and another lane's read WITHOUT lds_settle() in
// between sees lane 0 run ahead of lane 63 here: the reader gets the old contents.  A spot that shows up this way is a
// finding to judge, not a licence to change the kernel.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../lockstep.h"

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static __attribute__((section("xm_lds")))

typedef void *hipStream_t;
typedef ls::dim3 dim3;

struct uint2 { uint32_t x, y; } __attribute__((aligned(8)));
struct uint4 { uint32_t x, y, z, w; } __attribute__((aligned(16)));
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }

#define threadIdx (ls::cur->tid)
#define blockIdx (ls::g_block)
#define gridDim (ls::g_grid)

#define __syncthreads() ls::syncthreads(__builtin_LINE())
#define __ballot(p) ls::ballot((p), __builtin_LINE())
#define __shfl_xor(v, m, w) ls::shfl_xor((v), (m), (w), __builtin_LINE())
#define __builtin_amdgcn_readlane(v, l) ls::readlane((v), (l), __builtin_LINE())
#define __builtin_amdgcn_readfirstlane(v) ls::readfirstlane((v), __builtin_LINE())
#define __builtin_amdgcn_ds_bpermute(a, v) ls::ds_bpermute((a), (v), __builtin_LINE())
#define __builtin_amdgcn_update_dpp(o, s, c, rm, bm, bc) ls::update_dpp((o), (s), (c), (rm), (bm), (bc), __builtin_LINE())
#define __builtin_amdgcn_mbcnt_lo(m, a) ls::mbcnt_lo((m), (a))
#define __builtin_amdgcn_mbcnt_hi(m, a) ls::mbcnt_hi((m), (a))
#define __builtin_amdgcn_ubfe(s, o, w) ls::ubfe((s), (o), (w))

static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
static inline int32_t __mul24(int32_t a, int32_t b)
{
    const int64_t x = (int32_t)((uint32_t)a << 8) >> 8, y = (int32_t)((uint32_t)b << 8) >> 8;
    return (int32_t)(uint32_t)(uint64_t)(x * y);
}

static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
