// xm_bamframe.h -- the frames of BAM outputs written as BGZF members of stored blocks, shared by the two device front ends
// (xm_bamdev.hip: xm_bamdev_fetch_bins_bam, records gathered as they stand; xm_strip.hip: xm_strip_fetch_bins_bam, records encoded from
// SAM lines): the layout of the members from the size scan's bin starts, their descriptors for the CRC kernel, and the frames
// themselves.  Kernels in an anonymous namespace, as in xm_gather.h: each translation unit that includes this gets its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xenomapper_bgzf.h"

namespace {

constexpr uint32_t BGZF_HEAD = 18, STORED_HEAD = 5, BGZF_TAIL = 8, BGZF_FRAME = BGZF_HEAD + STORED_HEAD + BGZF_TAIL;

// what O1 leaves for O2: F_b (b = 0..6; [7] = the framed total) and the index of every bin's first member ([7] = how many there are)
struct BamLayout { uint32_t frame_start[8], member_start[8]; };

__device__ __forceinline__ void bam_layout_of(const uint32_t *__restrict__ starts, uint32_t P, BamLayout &l)
{
    uint32_t f = 0, m = 0;
#pragma unroll
    for (uint32_t b = 0; b < 7u; ++b) {
        l.frame_start[b] = f; l.member_start[b] = m;
        const uint32_t len = starts[b + 1u] - starts[b], members = (len + P - 1u) / P;
        f += len + members * BGZF_FRAME;
        m += members;
    }
    l.frame_start[7] = f; l.member_start[7] = m;
}

// O1: a lane per member: its descriptor for the CRC kernel (out_off: the payload's first byte in the framed stream, isize: its bytes)
__global__ void __launch_bounds__(256)
bam_layout_kernel(const uint32_t *__restrict__ starts, uint32_t P, uint32_t n_members, BamLayout *__restrict__ layout,
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
    d.cdata_off = 0; d.cdata_len = 0;
    d.out_off = (uint64_t)l.frame_start[b] + (uint64_t)k * (P + BGZF_FRAME) + BGZF_HEAD + STORED_HEAD;
    d.isize = left < P ? left : P;
    members[m] = d;
}

// O3: a lane per member: the gzip header with the BC subfield (BSIZE = member size - 1), the stored block's header, CRC-32 and ISIZE
__global__ void __launch_bounds__(256)
bam_frame_kernel(const xm_bgzf_block *__restrict__ members, const uint32_t *__restrict__ crc, uint32_t n_members, uint8_t *__restrict__ out,
                 uint32_t out_cap)
{
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m >= n_members) return;
    const xm_bgzf_block d = members[m];
    const uint32_t len = d.isize, bsize = len + BGZF_FRAME - 1u;
    if (d.out_off < BGZF_HEAD + STORED_HEAD || d.out_off + len + BGZF_TAIL > out_cap || len > 0xFFFFu - BGZF_FRAME + 1u) return;
    uint8_t *h = out + d.out_off - (BGZF_HEAD + STORED_HEAD);
    const uint8_t head[BGZF_HEAD + STORED_HEAD] = {
        0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8),
        1, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
#pragma unroll
    for (uint32_t k = 0; k < BGZF_HEAD + STORED_HEAD; ++k) h[k] = head[k];
    uint8_t *t = out + d.out_off + len;
    const uint32_t c = crc[m];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { t[k] = (uint8_t)(c >> (8u * k)); t[4u + k] = (uint8_t)(len >> (8u * k)); }
}

}  // namespace
