// xm_bgzf_pack.h -- the kernel that makes complete BGZF members of deflated streams, for the two places that frame what
// xm_bgzf_deflate_dev wrote: xm_bgzf_compress (xm_deflate.hip), xm_bamdev_fetch_bins_bamz (xm_bamdev.hip) and xm_strip_fetch_bins_bamz
// (xm_strip.hip).  In an anonymous namespace like xm_gather.h: each translation unit that includes this gets its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xenomapper_bgzf.h"

namespace {

typedef uint32_t pack_v4u32 __attribute__((ext_vector_type(4)));
typedef uint32_t pack_v4u32_any __attribute__((ext_vector_type(4), aligned(1)));

// A wave per member: the 18-byte header of bam_frame_kernel (xm_bamdev.hip) with BSIZE = clen + 25, the stream 16 bytes per lane from
// its slot (aligned loads; the member begins wherever the scan put it), CRC-32 and ISIZE.
__global__ void __launch_bounds__(64)
bgzf_pack_kernel(const uint8_t *__restrict__ comp, const xm_bgzf_block *__restrict__ blocks, const uint32_t *__restrict__ clen,
                 const uint32_t *__restrict__ crc, const uint64_t *__restrict__ member_off, uint32_t n_blocks, uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blocks) return;
    const xm_bgzf_block d = blocks[b];
    const uint32_t n = clen[b], bsize = n + 25u;
    uint8_t *m = out + member_off[b];
    if (lane < 18u) {
        const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
        m[lane] = head[lane];
    }
    const uint8_t *src = comp + d.cdata_off;
    uint8_t *body = m + 18u;
    for (uint32_t i = 16u * lane; i + 16u <= n; i += 16u * 64u)
        *reinterpret_cast<pack_v4u32_any *>(body + i) = *reinterpret_cast<const pack_v4u32 *>(src + i);
    const uint32_t rest = n & ~15u;
    if (rest + lane < n) body[rest + lane] = src[rest + lane];
    if (lane < 8u) {
        const uint32_t v = lane < 4u ? crc[b] : d.isize;
        body[n + lane] = (uint8_t)(v >> (8u * (lane & 3u)));
    }
}

}  // namespace
