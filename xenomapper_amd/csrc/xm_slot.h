// xm_slot.h -- the host half both device front ends (xm_strip.hip: SAM text, xm_bamdev.hip: BAM) share from the point where a
// slot's score columns are in HBM: error text and allocation, the fused classify pass on a slot and its read-back, the column
// downloads, and the gather's placement and hand-off around the kernels of xm_gather.h.  Host code only, in an anonymous namespace
// like xm_gather.h: each translation unit that includes this gets its own.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/xenomapper_hip.h"
#include "xm_gather.h"
#include "xm_pinned.h"

namespace {

// ---- what xm_strip and xm_bamdev both begin with ---------------------------------------------------------------------
struct FrontEnd {
    xm_ctx *ctx = nullptr;
    int device = 0;
    std::mutex error_lock;                             // the two slots are driven by two threads
    std::string last_error;
};

int fail(FrontEnd *s, hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    if (s) {
        std::lock_guard<std::mutex> hold(s->error_lock);
        s->last_error = buf;
    }
    (void)hipGetLastError();        // reported here: a later launch check on this thread must not find it again
    return e == hipErrorOutOfMemory ? XM_ERR_OOM : XM_ERR_HIP;
}

#define XMF_HIP(s, call)                                   \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return fail((s), e_, #call); \
    } while (0)

#define XMF_TRY(expr) do { int rc_ = (expr); if (rc_ != XM_OK) return rc_; } while (0)

void take_ctx_error(FrontEnd *s)                       // a call into the context failed: its error text becomes the front end's
{
    std::lock_guard<std::mutex> hold(s->error_lock);
    s->last_error = xm_last_hip_error(s->ctx);
}

const char *last_error_text(const FrontEnd *s)
{
    // the other slot's thread may be assigning the text: copied under the lock into a buffer of the calling thread
    static thread_local std::string mine;
    if (!s) return "";
    std::lock_guard<std::mutex> hold(const_cast<FrontEnd *>(s)->error_lock);
    mine = s->last_error;
    return mine.c_str();
}

template <typename T> void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }
template <typename T> void hfree(T *&p) { if (p) { (void)xmpin::host_free(p); p = nullptr; } }

template <typename T> int dalloc(FrontEnd *s, T *&p, size_t count)
{
    dfree(p);
    XMF_HIP(s, hipMalloc((void **)&p, std::max<size_t>(count, 16) * sizeof(T)));
    return XM_OK;
}
template <typename T> int halloc(FrontEnd *s, T *&p, size_t count)
{
    hfree(p);
    XMF_HIP(s, xmpin::host_malloc((void **)&p, std::max<size_t>(count, 16) * sizeof(T)));
    return XM_OK;
}

// Everything queued on `st` has ended, and no launch failed.  sleep_on: a blocking-sync event the waiting thread sleeps on instead
// of spinning on a core (the BAM side, for the reason written at its Slot::ev_wait); null: the stream is synchronised (the SAM side).
int wait_for(FrontEnd *s, hipStream_t st, hipEvent_t sleep_on)
{
    if (sleep_on) XMF_HIP(s, hipEventRecord(sleep_on, st));
    XMF_HIP(s, sleep_on ? hipEventSynchronize(sleep_on) : hipStreamSynchronize(st));
    XMF_HIP(s, hipGetLastError());
    return XM_OK;
}

// the size scan of xm_gather.h over v[0, n): place[i] = the sizes in front of item i, *total = all of them (three launches)
template <bool ALL>
void scan_sizes(hipStream_t st, const uint32_t *v, uint32_t n, uint32_t *part, uint32_t *place, uint32_t *total)
{
    const uint32_t n_part = (n + SCAN_TILE - 1u) / SCAN_TILE;
    size_sum_kernel<<<n_part, 256, 0, st>>>(v, n, part);
    part_scan_kernel<<<1, 1024, 0, st>>>(part, n_part, total);
    size_place_kernel<ALL><<<n_part, 256, 0, st>>>(v, n, part, place);
}

// ---- the fused classify pass on a slot's columns ----------------------------------------------------------------------
struct CigCols { const int32_t *nm; const uint8_t *cnt; const uint32_t *tile, *ops; };      // one file's packed CIGAR columns

struct ClassifyOut {
    int32_t *d_col[4] = {nullptr, nullptr, nullptr, nullptr};      // as1, xs1, as2, xs2 (CIGAR mode: the front end says where NM is)
    uint64_t *d_bits = nullptr;                                     // the unit mask
    uint8_t *d_code = nullptr, *d_bins4 = nullptr, *h_code = nullptr;
    uint32_t *d_idx = nullptr, *h_idx = nullptr;
    uint32_t *d_range = nullptr, *h_range = nullptr;                // CIGAR mode: a synthesised score left int32
    uint64_t *d_off_counts = nullptr, *h_off_counts = nullptr;      // 8 bin offsets ([7]: the units) + 64 counts
    bool classified = false;                           // the fused pass has run on the columns (its compact category stream is in d_bins4)

    hipError_t create()                                // the parts whose size never changes
    {
        hipError_t e = hipMalloc((void **)&d_off_counts, 72 * sizeof(uint64_t));
        if (e == hipSuccess) e = xmpin::host_malloc((void **)&h_off_counts, 72 * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_range, 4 * sizeof(uint32_t));
        if (e == hipSuccess) e = xmpin::host_malloc((void **)&h_range, 4 * sizeof(uint32_t));
        return e;
    }
    void destroy() { dfree(d_off_counts); hfree(h_off_counts); dfree(d_range); hfree(h_range); }

    int grow(FrontEnd *s, uint64_t records)            // the per-record parts
    {
        const size_t n = (size_t)records + 64;
        for (int c = 0; c < 4; ++c) XMF_TRY(dalloc(s, d_col[c], n));
        XMF_TRY(dalloc(s, d_bits, n / 64 + 2)); XMF_TRY(dalloc(s, d_bins4, (size_t)XM_BINS4_BYTES(records) + 16));
        XMF_TRY(dalloc(s, d_code, n)); XMF_TRY(dalloc(s, d_idx, n));
        XMF_TRY(halloc(s, h_code, n)); XMF_TRY(halloc(s, h_idx, n));
        return XM_OK;
    }
    void release()
    {
        for (int c = 0; c < 4; ++c) dfree(d_col[c]);
        dfree(d_bits); dfree(d_code); dfree(d_bins4); dfree(d_idx); hfree(h_code); hfree(h_idx);
    }

    // The fused pass on the first n (> 0) records, on `st` and waited for: code, the index lists and the 72 words on the host.
    // cig: both files' packed CIGAR columns, which the classify kernel makes AS of (--cigar_scores), or null: the columns hold AS.
    int run_fused(FrontEnd *s, hipStream_t st, int mode, uint64_t n, int32_t min_score_floor, const CigCols *cig,
                  uint64_t bin_offsets[8], uint64_t counts[64])
    {
        int rc;
        if (cig) {
            XMF_HIP(s, hipMemsetAsync(d_range, 0, sizeof(uint32_t), st));
            const CigCols &a = cig[0], &b = cig[1];
            rc = xm_classify_compact_cigar_packed_dev(s->ctx, st, mode, n, a.nm, a.cnt, a.tile, a.ops, d_col[1], b.nm, b.cnt, b.tile, b.ops,
                                                      d_col[3], d_bits, min_score_floor, d_code, d_bins4, d_range, d_idx, d_off_counts,
                                                      d_off_counts + 8);
        } else {
            rc = xm_classify_compact_dev(s->ctx, st, mode, n, d_col[0], d_col[1], d_col[2], d_col[3], d_bits, min_score_floor, d_code,
                                         d_bins4, d_idx, d_off_counts, d_off_counts + 8);
        }
        if (rc != XM_OK) { take_ctx_error(s); return rc; }
        XMF_HIP(s, hipMemcpyAsync(h_code, d_code, n, hipMemcpyDeviceToHost, st));
        XMF_HIP(s, hipMemcpyAsync(h_off_counts, d_off_counts, 72 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (cig) XMF_HIP(s, hipMemcpyAsync(h_range, d_range, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        XMF_HIP(s, hipStreamSynchronize(st));
        if (cig && *h_range != 0u) return XM_ERR_RANGE;               // a score left int32: the caller's text rules decide
        const uint64_t units = h_off_counts[7];
        if (units > n) return XM_ERR_HIP;
        if (units) {
            XMF_HIP(s, hipMemcpyAsync(h_idx, d_idx, units * 4, hipMemcpyDeviceToHost, st));
            XMF_HIP(s, hipStreamSynchronize(st));
        }
        std::memcpy(bin_offsets, h_off_counts, 8 * sizeof(uint64_t));
        std::memcpy(counts, h_off_counts + 8, 64 * sizeof(uint64_t));
        classified = true;
        return XM_OK;
    }

    // the first n (> 0) entries of the score columns and the unit mask to the caller's arrays (each may be null)
    int columns_to_host(FrontEnd *s, hipStream_t st, uint64_t n, int32_t *as1, int32_t *xs1, int32_t *as2, int32_t *xs2, uint64_t *unit_bits)
    {
        int32_t *dst[4] = {as1, xs1, as2, xs2};
        for (int c = 0; c < 4; ++c)
            if (dst[c]) XMF_HIP(s, hipMemcpyAsync(dst[c], d_col[c], n * 4, hipMemcpyDeviceToHost, st));
        if (unit_bits) XMF_HIP(s, hipMemcpyAsync(unit_bits, d_bits, (n + 63) / 64 * 8, hipMemcpyDeviceToHost, st));
        XMF_HIP(s, hipStreamSynchronize(st));
        return XM_OK;
    }
};

// ---- the gather: where every unit's bytes go, and the finished stream's way home ----------------------------------------
// The gather's state words, the same in both front ends, as offsets into a block of GS_WORDS uint32 that begins on an 8-byte
// boundary (GS_TOTAL64 is added to by 64-bit atomics).  The front end clears words [GS_FLAG, GS_WORDS) in front of its sizing
// kernels; those set the flag and sum the sizes in 64 bits, place_units fills in the rest.
enum {
    GS_PAD = 0,          // not the gather's (it keeps GS_TOTAL64 aligned)
    GS_FLAG = 1,         // the sizing kernels met something the device does not print: the window is the host's
    GS_TOTAL = 2,        // the scan's total, in 32 bits: bin_start_kernel's total_and_wrapped[0]
    GS_WRAP = 3,         // the word behind it: kept for a wrap mark, which no kernel sets today (GS_TOTAL64 is the check)
    GS_STARTS = 4,       // [8]: where bin b's bytes begin, b = 0..6; [7] = the total
    GS_TOTAL64 = 12,     // two words: the sizes summed in 64 bits -- the 32-bit places hold only if this fits the buffer
    GS_WORDS = 14
};
constexpr size_t GS_LIVE_BYTES = (GS_WORDS - GS_FLAG) * sizeof(uint32_t);       // what is cleared and read back

struct Placed { uint32_t flag; uint64_t total; uint32_t starts[8]; };           // what place_units read back

struct GatherPlan {
    uint32_t *d_usize = nullptr, *d_uplace = nullptr, *d_upart = nullptr;      // per unit: its bytes, where they go; the scan's partials
    uint64_t unit_cap = 0;

    int reserve_units(FrontEnd *s, uint64_t records)
    {
        if (records <= unit_cap) return XM_OK;
        unit_cap = 0;
        const size_t n = (size_t)records + 64;
        XMF_TRY(dalloc(s, d_usize, n)); XMF_TRY(dalloc(s, d_uplace, n)); XMF_TRY(dalloc(s, d_upart, n / SCAN_TILE + 8));
        unit_cap = records;
        return XM_OK;
    }
    void free_units() { dfree(d_usize); dfree(d_uplace); dfree(d_upart); unit_cap = 0; }

    // d_usize[0, n_units) is filled: places every unit (they are in bin order: the scan IS the layout of the six outputs back to back),
    // notes where each bin begins, reads the state block back and waits for it (wait_for's two ways)
    int place_units(FrontEnd *s, hipStream_t st, uint32_t n_units, const unsigned long long *d_off, uint32_t *state_dev,
                    uint32_t *state_host, hipEvent_t sleep_on, Placed &out)
    {
        scan_sizes<true>(st, d_usize, n_units, d_upart, d_uplace, state_dev + GS_TOTAL);
        bin_start_kernel<<<1, 64, 0, st>>>(d_uplace, d_off, n_units, state_dev + GS_TOTAL, state_dev + GS_STARTS);
        XMF_HIP(s, hipMemcpyAsync(state_host + GS_FLAG, state_dev + GS_FLAG, GS_LIVE_BYTES, hipMemcpyDeviceToHost, st));
        XMF_TRY(wait_for(s, st, sleep_on));
        out.flag = state_host[GS_FLAG];
        std::memcpy(&out.total, state_host + GS_TOTAL64, sizeof out.total);
        for (int k = 0; k < 8; ++k) out.starts[k] = state_host[GS_STARTS + k];
        return XM_OK;
    }

    // `bytes` of the finished stream at d go to h (page-locked, device-mapped) on the copy stream, behind everything queued on
    // `st` (ev_filled) and beside whatever `st` does next; ev_out marks the copy's end
    static int send_home(FrontEnd *s, hipStream_t st, hipStream_t copy_stream, hipEvent_t ev_filled, hipEvent_t ev_out, const uint8_t *d,
                         uint8_t *h, uint64_t bytes)
    {
        XMF_HIP(s, hipEventRecord(ev_filled, st));
        XMF_HIP(s, hipStreamWaitEvent(copy_stream, ev_filled, 0));
        out_copy(d, h, bytes, copy_stream);
        XMF_HIP(s, hipEventRecord(ev_out, copy_stream));
        XMF_HIP(s, hipGetLastError());
        return XM_OK;
    }
};

}  // namespace
