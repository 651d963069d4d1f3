// xm_deflate.hip -- BGZF blocks deflated on the GPU (include/xenomapper_bgzf.h): the launch around xm_deflate_core.h and the
// host-buffer call on top of it and of the kernel that packs the streams into BGZF members (xm_bgzf_pack.h).  Stand-alone beside xm_bamdev_*, as
// xm_bgzf_inflate_dev and xm_bgzf_crc32_dev are.
//
// Launch shape, as the inflate launch: one workgroup = one wave = one chain, persistent, taking block numbers from a counter.
// A chain holds ~22 KB of LDS (xmd::ChainMem: the 16 KB hash table, histograms, the Huffman tree) and 255 KB of device scratch
// (one word per input byte: the match candidates of phase M, read three times by the walks of P and E).  The scratch decides
// how many chains there are: 1024 of them are 255 MB, the ceiling the header promises for xm_bgzf_deflate_work_bytes(); the LDS
// would allow 7 per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/xenomapper_bgzf.h"
#include "xm_bgzf_pack.h"                // bgzf_pack_kernel: the streams framed as BGZF members
#include "xm_deflate_core.h"

static_assert(XMB_DEFLATE_MAX_ISIZE == xmd::MAX_ISIZE, "the header's limit is the core's");

namespace {

constexpr uint64_t WORK_HEAD = 256;                                         // the counter, and the scratch behind it stays aligned
constexpr uint64_t CHAIN_SCRATCH = (uint64_t)xmd::SCRATCH_WORDS * 4u;       // bytes (a multiple of 16)
constexpr uint64_t MAX_CHAINS = 1024;
constexpr uint64_t CHAINS_PER_CU = 7;                                       // what the LDS allows (160 KB per CU)
static_assert(WORK_HEAD + MAX_CHAINS * CHAIN_SCRATCH <= (256ull << 20), "xm_bgzf_deflate_work_bytes() stays within 256 MiB");
static_assert(CHAIN_SCRATCH % 16u == 0, "a chain's scratch is read 16 bytes at a time");

__global__ void __launch_bounds__(64)
deflate_kernel(const uint8_t *__restrict__ in, const xm_bgzf_block *__restrict__ blocks, uint32_t n_blocks, uint8_t *__restrict__ comp,
               uint32_t *__restrict__ clen, uint32_t *__restrict__ status, uint32_t *__restrict__ counter, uint32_t *__restrict__ scratch)
{
    __shared__ xmd::ChainMem mem;
    uint32_t *mine = scratch + (uint64_t)blockIdx.x * xmd::SCRATCH_WORDS;
    const uint32_t lane = threadIdx.x;
    for (;;) {
        // The chain's next block.  EVERY lane takes part in the fetch (lane 0 adds 1, the others 0; the compiler makes one atomic of
        // it) and the block number is lane 0's result, read with v_readfirstlane: nothing here, and nothing at the loop's end, is
        // done by "lane 0 only".  It was, at first -- lane 0 fetched, left the number in LDS, the others read it behind a wave
        // barrier, and lane 0 alone stored status and clen -- and that launch never came back: the compiler joined the two
        // `if (lane == 0)` across the back edge into a path of lane 0's own, which made TWO loops of this one; lanes 1 .. 63 stayed
        // in the inner one and read the old number from LDS for ever, while lane 0 waited outside for them to leave it (the ISA:
        // the atomic in the depth-1 header, the whole body in a depth-2 loop that lane 0 alone exits).  A wave barrier is no
        // reconvergence point; rule R1 of xm_deflate_core.h -- no lane waits for another -- holds for this loop too.
        // (Every chain ends here once the counter has passed n_blocks: the grid always drains.)
        const uint32_t b = __builtin_amdgcn_readfirstlane(atomicAdd(counter, lane == 0u ? 1u : 0u));
        if (b >= n_blocks) break;
        const xm_bgzf_block d = blocks[b];
        uint32_t st = XMB_OK;
        if (d.isize > XMB_DEFLATE_MAX_ISIZE) st = XMB_DEFLATE_ERR_ISIZE;
        else if (d.cdata_len < XMB_DEFLATE_BOUND(d.isize)) st = XMB_DEFLATE_ERR_CAPACITY;
        else if (d.cdata_off & 15u) st = XMB_DEFLATE_ERR_ALIGN;
        uint32_t len = 0;
        if (st == XMB_OK) len = xmd::deflate_block(&mem, in + d.out_off, d.isize, comp + d.cdata_off, mine);
        // all lanes store the same two words (len is the same in every lane: deflate_block computes it from LDS)
        status[b] = st;
        clen[b] = __builtin_amdgcn_readfirstlane(len);
    }
}

struct DevBuf {                                     // freed when the call returns, whichever way
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

}  // namespace

extern "C" {

uint64_t xm_bgzf_deflate_work_bytes(void) { return WORK_HEAD + MAX_CHAINS * CHAIN_SCRATCH; }

int xm_bgzf_deflate_dev(xm_ctx *ctx, void *stream, const uint8_t *in, const xm_bgzf_block *blocks, uint64_t n_blocks,
                        uint8_t *comp, uint32_t *clen, uint32_t *status, void *work, uint64_t work_bytes)
{
    if (!ctx || n_blocks > 0x7FFFFFFFull) return XM_ERR_INVALID_ARG;
    if (n_blocks == 0) return XM_OK;
    if (!in || !blocks || !comp || !clen || !status || !work || ((uintptr_t)comp & 15u) || ((uintptr_t)blocks & 7u) ||
        ((uintptr_t)work & 15u) || work_bytes < WORK_HEAD + CHAIN_SCRATCH)
        return XM_ERR_INVALID_ARG;
    int n_cu = 0;
    if (xm_ctx_device_info(ctx, &n_cu, nullptr, 0) != XM_OK || n_cu <= 0) return XM_ERR_INVALID_ARG;
    uint64_t chains = (work_bytes - WORK_HEAD) / CHAIN_SCRATCH;             // what the scratch given holds,
    if (chains > MAX_CHAINS) chains = MAX_CHAINS;
    if (chains > (uint64_t)n_cu * CHAINS_PER_CU) chains = (uint64_t)n_cu * CHAINS_PER_CU;   // what the chip holds at once,
    if (chains > n_blocks) chains = n_blocks;                               // what there is to do
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(work, 0, sizeof(uint32_t), st) != hipSuccess) return XM_ERR_HIP;
    deflate_kernel<<<(uint32_t)chains, 64, 0, st>>>(in, blocks, (uint32_t)n_blocks, comp, clen, status, static_cast<uint32_t *>(work),
                                                    reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(work) + WORK_HEAD));
    return hipGetLastError() == hipSuccess ? XM_OK : XM_ERR_HIP;
}

int xm_bgzf_compress(xm_ctx *ctx, const uint8_t *data, uint64_t len, uint32_t block_payload, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_len)
{
    if (!ctx || !out_len || (len && (!data || !out))) return XM_ERR_INVALID_ARG;
    const uint32_t P = block_payload ? block_payload : XMB_DEFLATE_MAX_ISIZE;
    if (P < 64u || P > XMB_DEFLATE_MAX_ISIZE) return XM_ERR_INVALID_ARG;
    if (out_cap < XMB_COMPRESS_BOUND(len, (uint64_t)P)) return XM_ERR_INVALID_ARG;
    *out_len = 0;
    if (len == 0) return XM_OK;
    // Windows: at most 64 MiB of input and 2^20 blocks at a time -- the device buffers of a window are then 64 MiB of input, as
    // much again and 21 bytes a block for the slots, the same for the members, and the chains' scratch.
    const uint64_t slot = ((uint64_t)P + 5u + 15u) & ~15ull;
    uint64_t win_blocks = (64ull << 20) / P;
    if (win_blocks > (1ull << 20)) win_blocks = 1ull << 20;
    if (win_blocks < 1) win_blocks = 1;
    const uint64_t total_blocks = (len + P - 1u) / P;
    if (win_blocks > total_blocks) win_blocks = total_blocks;
    const uint64_t win_bytes = win_blocks * P;
    uint64_t chains = win_blocks < MAX_CHAINS ? win_blocks : MAX_CHAINS;
    const uint64_t work_bytes = WORK_HEAD + chains * CHAIN_SCRATCH;
    DevBuf d_in, d_blocks, d_comp, d_clen, d_status, d_crc, d_off, d_out, d_work;
    if (!d_in.alloc(win_bytes + 16u) || !d_blocks.alloc(win_blocks * sizeof(xm_bgzf_block)) || !d_comp.alloc(win_blocks * slot) ||
        !d_clen.alloc(win_blocks * 4u) || !d_status.alloc(win_blocks * 4u) || !d_crc.alloc(win_blocks * 4u) ||
        !d_off.alloc(win_blocks * 8u) || !d_out.alloc(win_bytes + 31u * win_blocks) || !d_work.alloc(work_bytes))
        return XM_ERR_OOM;
    std::vector<xm_bgzf_block> blocks(win_blocks);
    std::vector<uint32_t> clen(win_blocks), status(win_blocks);
    std::vector<uint64_t> off(win_blocks);
    hipStream_t st = nullptr;
    uint64_t written = 0;
    for (uint64_t at = 0; at < len; at += win_bytes) {
        const uint64_t bytes = len - at < win_bytes ? len - at : win_bytes, nb = (bytes + P - 1u) / P;
        for (uint64_t b = 0; b < nb; ++b) {
            blocks[b].cdata_off = b * slot;
            blocks[b].cdata_len = (uint32_t)slot;
            blocks[b].out_off = b * P;
            blocks[b].isize = (uint32_t)(bytes - b * P < P ? bytes - b * P : P);
        }
        if (hipMemcpyAsync(d_in.p, data + at, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_blocks.p, blocks.data(), nb * sizeof(xm_bgzf_block), hipMemcpyHostToDevice, st) != hipSuccess)
            return XM_ERR_HIP;
        int rc = xm_bgzf_deflate_dev(ctx, st, d_in.as<uint8_t>(), d_blocks.as<xm_bgzf_block>(), nb, d_comp.as<uint8_t>(),
                                     d_clen.as<uint32_t>(), d_status.as<uint32_t>(), d_work.p, work_bytes);
        if (rc == XM_OK) rc = xm_bgzf_crc32_dev(ctx, st, d_in.as<uint8_t>(), d_blocks.as<xm_bgzf_block>(), nb, d_crc.as<uint32_t>());
        if (rc != XM_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (hipMemcpyAsync(clen.data(), d_clen.p, nb * 4u, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(status.data(), d_status.p, nb * 4u, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return XM_ERR_HIP;
        // the members' places: the exclusive scan of clen + 26 (on the host: the call blocks anyway)
        uint64_t total = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            if (status[b] != XMB_OK || clen[b] > XMB_DEFLATE_BOUND(blocks[b].isize)) return XM_ERR_HIP;    // (the slots are made to fit)
            off[b] = total;
            total += (uint64_t)clen[b] + 26u;
        }
        if (written + total > out_cap) return XM_ERR_INVALID_ARG;           // (the bound was checked: cannot happen)
        if (hipMemcpyAsync(d_off.p, off.data(), nb * 8u, hipMemcpyHostToDevice, st) != hipSuccess) return XM_ERR_HIP;
        bgzf_pack_kernel<<<(uint32_t)nb, 64, 0, st>>>(d_comp.as<uint8_t>(), d_blocks.as<xm_bgzf_block>(), d_clen.as<uint32_t>(),
                                                      d_crc.as<uint32_t>(), d_off.as<uint64_t>(), (uint32_t)nb, d_out.as<uint8_t>());
        if (hipGetLastError() != hipSuccess) return XM_ERR_HIP;
        if (hipMemcpyAsync(out + written, d_out.p, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return XM_ERR_HIP;
        written += total;
    }
    *out_len = written;
    return XM_OK;
}

}  // extern "C"
