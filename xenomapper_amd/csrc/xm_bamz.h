// xm_bamz.h -- the member descriptors and the place scan of COMPRESSED BAM outputs, shared by the two device front ends
// (xm_bamdev.hip: xm_bamdev_fetch_bins_bamz, records gathered as they stand; xm_strip.hip: xm_strip_fetch_bins_bamz, records encoded from
// SAM lines).  Both gather their payloads without frames, bin b's bytes from starts[b] on, and launch the kernels below around
// xm_bgzf_deflate_dev; bgzf_pack_kernel (xm_bgzf_pack.h) comes behind them.  Kernels in an anonymous namespace, as in xm_bamframe.h: each
// translation unit that includes this gets its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xenomapper_bgzf.h"
#include "xm_bamframe.h"

namespace {

// ---- Z: the six outputs as compressed BAM (xm_bamdev_fetch_bins_bamz): the same payloads, each member deflated -----------------------
// O's scan and O's members, but the payloads are gathered WITHOUT frames into a buffer of their own (Z2 = O2 with FRAMED = false:
// bin b's bytes from S_b on), member m's stream is made by xm_bgzf_deflate_dev in a slot of its own (m * slot, slot = P + 5 rounded up
// to 16: what a stream never exceeds), and only then is it known where a member lies in the output: Z4 scans the streams' lengths + 26,
// Z5 (bgzf_pack_kernel, xm_bgzf_pack.h) moves every stream between its header and its trailer.
// Z1: a lane per member: its descriptor for the encoder and the CRC kernel; lane 0 leaves the bins' first members for Z4
__global__ void __launch_bounds__(256)
bamz_layout_kernel(const uint32_t *__restrict__ starts, uint32_t P, uint32_t slot, uint32_t n_members, BamLayout *__restrict__ layout,
                   xm_bgzf_block *__restrict__ members)
{
    BamLayout l;
    bam_layout_of(starts, P, l);
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m == 0u) *layout = l;
    if (m >= n_members || m >= l.member_start[7]) return;
    uint32_t b = 0;
#pragma unroll
    for (uint32_t k = 1; k < 7u; ++k) b += (l.member_start[k] <= m) ? 1u : 0u;
    const uint32_t k = m - l.member_start[b], len = starts[b + 1u] - starts[b], left = len - k * P;
    xm_bgzf_block d;
    d.cdata_off = (uint64_t)m * slot; d.cdata_len = slot;
    d.out_off = (uint64_t)starts[b] + (uint64_t)k * P;
    d.isize = left < P ? left : P;
    members[m] = d;
}

// Z4: where every member goes: the exclusive scan of clen[m] + 26 (18 bytes of header, 8 of trailer) over the members, in ONE workgroup
// the way part_scan_kernel (xm_gather.h) scans the size scan's partials -- thread t sums the members [t per, (t + 1) per), per =
// ceil(n / 256), the 256 sums are scanned in LDS, and the thread walks its members again from its base: any number of members, one
// launch.  placed[b] = where bin b's first member lies (b = 0..6; a bin without members: where the next one's does), placed[7] = the
// total, placed[8] = the OR of the members' status -- with XMB_DEFLATE_ERR_CAPACITY for a length no stream may have, which is then
// set to 0 so that Z5 writes nothing but that member's frame.
constexpr uint32_t BAMZ_PLACE_THREADS = 256;      // (members are few: 4 000 in a window of 256 MB at the default payload)
__global__ void __launch_bounds__(BAMZ_PLACE_THREADS)
bamz_place_kernel(const xm_bgzf_block *__restrict__ members, uint32_t *__restrict__ clen, const uint32_t *__restrict__ status, uint32_t n_members,
                  const BamLayout *__restrict__ layout, unsigned long long *__restrict__ member_off, unsigned long long *__restrict__ placed)
{
    __shared__ unsigned long long sh[BAMZ_PLACE_THREADS];
    __shared__ uint32_t any_status;
    const uint32_t t = threadIdx.x, per = (n_members + BAMZ_PLACE_THREADS - 1u) / BAMZ_PLACE_THREADS;
    const uint32_t a = min(t * per, n_members), e = min(a + per, n_members);
    if (t == 0u) any_status = 0u;
    __syncthreads();
    unsigned long long s = 0;
    uint32_t st = 0;
    for (uint32_t k = a; k < e; ++k) {
        uint32_t c = clen[k];
        const uint32_t bad = status[k] | (c > XMB_DEFLATE_BOUND(members[k].isize) ? XMB_DEFLATE_ERR_CAPACITY : 0u);
        if (bad) { c = 0u; clen[k] = 0u; }
        st |= bad;
        s += c + (BGZF_HEAD + BGZF_TAIL);
    }
    if (st) atomicOr(&any_status, st);
    sh[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < BAMZ_PLACE_THREADS; d <<= 1) {
        const unsigned long long x = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    uint32_t first[7];
#pragma unroll
    for (uint32_t b = 0; b < 7u; ++b) first[b] = layout->member_start[b];
    unsigned long long run = sh[t] - s;
    for (uint32_t k = a; k < e; ++k) {
        member_off[k] = run;
#pragma unroll
        for (uint32_t b = 0; b < 7u; ++b)
            if (first[b] == k) placed[b] = run;
        run += clen[k] + (BGZF_HEAD + BGZF_TAIL);
    }
    if (t == BAMZ_PLACE_THREADS - 1u) {
        const unsigned long long total = sh[BAMZ_PLACE_THREADS - 1u];
#pragma unroll
        for (uint32_t b = 0; b < 7u; ++b)
            if (first[b] >= n_members) placed[b] = total;
        placed[7] = total;
        placed[8] = any_status;
    }
}

}  // namespace
