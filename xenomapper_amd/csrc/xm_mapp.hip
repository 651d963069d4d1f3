// xm_mapp.hip -- the single-end mappability step on the GPU (C ABI in include/xenomapper_mappability.h), gfx950 only.
//
// Restates on the device the loop of single_end_mappability_from_sam (the reference's xenomapper/mappability.py:175-214) for one
// window of name-sorted SAM text and the state carried into it.  The kernels and their order are in xm_mapp_kernels.h; this file
// is the host half: the slots' buffers, the upload (M1 reads the page-locked staging buffer itself, as xm_strip.hip's S1 does) and
// the way the segment table and the values come home.
#include "../../include/xenomapper_mappability.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "xm_mapp_kernels.h"
#include "xm_slot.h"                       // FrontEnd, the error text, dalloc / halloc through xm_pinned.h

static_assert(XMM_R_NON_ASCII == xmm::R_NON_ASCII && XMM_R_SEPARATOR == xmm::R_SEPARATOR && XMM_R_FIELDS == xmm::R_FIELDS &&
              XMM_R_NAME_NUMBER == xmm::R_NAME_NUMBER && XMM_R_POS_NUMBER == xmm::R_POS_NUMBER &&
              XMM_R_NOT_SEQUENTIAL == xmm::R_NOT_SEQUENTIAL && XMM_DECLINED == xmm::S_DECLINED &&
              XMM_TOO_MANY_LINES == xmm::S_TOO_MANY_LINES && XMM_TOO_MANY_VALUES == xmm::S_TOO_MANY_VALUES,
              "the codes of xenomapper_mappability.h are xm_mapp_kernels.h's");
static_assert(sizeof(xm_mapp_segment) == sizeof(xmm::Seg) && offsetof(xm_mapp_segment, value_off) == offsetof(xmm::Seg, value_off) &&
              offsetof(xm_mapp_segment, last_pos) == offsetof(xmm::Seg, last_pos), "xm_mapp_segment is the kernels' row");

namespace {

struct Slot {
    uint64_t window_cap = 0, line_cap = 0, value_cap = 0;          // what the buffers hold
    uint64_t window = 0, max_lines = 0, max_values = 0;            // the last reserve's window and limits
    char *h_text = nullptr;
    uint8_t *d_text = nullptr;
    uint16_t *d_mask = nullptr;
    uint32_t *d_chunk_cnt = nullptr, *d_chunk_base = nullptr;
    uint32_t *d_lend = nullptr, *d_np = nullptr, *d_tlen = nullptr, *d_roff = nullptr, *d_rlen = nullptr, *d_seg_of = nullptr;
    uint8_t *d_flags = nullptr;
    uint32_t *d_part = nullptr, *d_part_base = nullptr;
    xmm::u64 *d_vpart = nullptr, *d_vbase = nullptr;
    xmm::Seg *d_segs = nullptr, *h_segs = nullptr;
    uint8_t *d_values = nullptr, *h_values = nullptr;
    uint8_t *d_key = nullptr;
    uint64_t key_cap = 0;
    uint32_t *d_state = nullptr;
    xmm::u64 *d_keys = nullptr, *d_summary = nullptr, *h_summary = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    uint64_t uploaded = 0;                                         // bytes of the staged window already on their way
    uint32_t marked = 0;                                           // chunks M1 has been launched for already
    bool state_cleared = false, upload_timed = false;
};

}  // namespace

struct xm_mapp : FrontEnd {
    Slot slot[XMM_SLOTS];
};

namespace {

void free_slot(Slot &sl)
{
    hfree(sl.h_text); dfree(sl.d_text); dfree(sl.d_mask); dfree(sl.d_chunk_cnt); dfree(sl.d_chunk_base);
    dfree(sl.d_lend); dfree(sl.d_np); dfree(sl.d_tlen); dfree(sl.d_roff); dfree(sl.d_rlen); dfree(sl.d_seg_of); dfree(sl.d_flags);
    dfree(sl.d_part); dfree(sl.d_part_base); dfree(sl.d_vpart); dfree(sl.d_vbase);
    dfree(sl.d_segs); hfree(sl.h_segs); dfree(sl.d_values); hfree(sl.h_values); dfree(sl.d_key);
    sl.window_cap = sl.line_cap = sl.value_cap = sl.key_cap = 0;
}

int grow_window(xm_mapp *m, Slot &sl, uint64_t bytes)
{
    if (bytes <= sl.window_cap) return XM_OK;
    const xmm::Sizes z = xmm::sizes_for(bytes, 1, 0);
    sl.window_cap = 0;
    XMF_TRY(halloc(m, sl.h_text, z.text));
    XMF_TRY(dalloc(m, sl.d_text, z.text));
    XMF_TRY(dalloc(m, sl.d_mask, z.mask16));
    XMF_TRY(dalloc(m, sl.d_chunk_cnt, z.chunk_cnt));
    XMF_TRY(dalloc(m, sl.d_chunk_base, z.chunk_cnt));
    sl.window_cap = z.text - xmm::TEXT_PAD;
    return XM_OK;
}

int grow_lines(xm_mapp *m, Slot &sl, uint64_t lines)
{
    if (lines <= sl.line_cap) return XM_OK;
    const xmm::Sizes z = xmm::sizes_for(0, lines, 0);
    sl.line_cap = 0;
    XMF_TRY(dalloc(m, sl.d_lend, z.lines)); XMF_TRY(dalloc(m, sl.d_np, z.lines)); XMF_TRY(dalloc(m, sl.d_tlen, z.lines));
    XMF_TRY(dalloc(m, sl.d_roff, z.lines)); XMF_TRY(dalloc(m, sl.d_rlen, z.lines)); XMF_TRY(dalloc(m, sl.d_seg_of, z.lines));
    XMF_TRY(dalloc(m, sl.d_flags, z.lines));
    XMF_TRY(dalloc(m, sl.d_part, z.tiles)); XMF_TRY(dalloc(m, sl.d_part_base, z.tiles));
    XMF_TRY(dalloc(m, sl.d_vpart, z.tiles)); XMF_TRY(dalloc(m, sl.d_vbase, z.tiles));
    XMF_TRY(dalloc(m, sl.d_segs, z.lines)); XMF_TRY(halloc(m, sl.h_segs, z.lines));
    sl.line_cap = lines;
    return XM_OK;
}

int grow_values(xm_mapp *m, Slot &sl, uint64_t values)
{
    if (values <= sl.value_cap && sl.d_values) return XM_OK;
    const xmm::Sizes z = xmm::sizes_for(0, 1, values);
    sl.value_cap = 0;
    XMF_TRY(dalloc(m, sl.d_values, z.values));
    XMF_TRY(halloc(m, sl.h_values, z.values));
    sl.value_cap = values;
    return XM_OK;
}

// M1 for chunks [sl.marked, upto_chunk) of the window, with `len` as the kernel is to see it
int mark_chunks(xm_mapp *m, Slot &sl, uint64_t len, uint32_t upto_chunk)
{
    if (!sl.state_cleared) {
        XMF_HIP(m, hipMemsetAsync(sl.d_state, 0, xmm::ST_WORDS * sizeof(uint32_t), sl.stream));
        sl.state_cleared = true;
    }
    if (upto_chunk <= sl.marked) return XM_OK;
    xmm::MarkArgs a;
    a.src = reinterpret_cast<const uint8_t *>(sl.h_text);
    a.copy = sl.d_text;
    a.mask16 = sl.d_mask; a.chunk_cnt = sl.d_chunk_cnt; a.state = sl.d_state;
    a.len = (uint32_t)len; a.chunk0 = sl.marked; a.n_chunks = upto_chunk - sl.marked;
    xmm::mark_kernel<<<a.n_chunks, xmm::MB, 0, sl.stream>>>(a);
    sl.marked = upto_chunk;
    return XM_OK;
}

bool bad_slot(const xm_mapp *m, int slot) { return !m || slot < 0 || slot >= XMM_SLOTS; }

}  // namespace

extern "C" {

int xmm_abi_version(void) { return XMM_ABI_VERSION; }

int xm_mapp_create(xm_ctx *ctx, int device_id, xm_mapp **out)
{
    if (!ctx || !out) return XM_ERR_INVALID_ARG;
    xm_mapp *m = new (std::nothrow) xm_mapp();
    if (!m) return XM_ERR_OOM;
    m->ctx = ctx;
    m->device = device_id;
    hipError_t e = hipSetDevice(device_id);
    for (int k = 0; k < XMM_SLOTS && e == hipSuccess; ++k) {
        Slot &sl = m->slot[k];
        // (the slots' streams are to work side by side, each on a hardware queue of its own: tried as xm_strip_create tries)
        hipStream_t before[XMM_SLOTS];
        for (int j = 0; j < k; ++j) before[j] = m->slot[j].stream;
        e = create_copy_stream(&sl.stream, before, k);
        for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&sl.ev[i]);
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_state, xmm::ST_WORDS * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_keys, xmm::K_WORDS * sizeof(xmm::u64));
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_summary, xmm::SUM_WORDS * sizeof(xmm::u64));
        if (e == hipSuccess) e = xmpin::host_malloc((void **)&sl.h_summary, xmm::SUM_WORDS * sizeof(xmm::u64));
    }
    if (e != hipSuccess) {
        xm_mapp_destroy(m);
        return e == hipErrorOutOfMemory ? XM_ERR_OOM : XM_ERR_HIP;
    }
    *out = m;
    return XM_OK;
}

int xm_mapp_destroy(xm_mapp *m)
{
    if (!m) return XM_ERR_INVALID_ARG;
    (void)hipSetDevice(m->device);
    for (int k = 0; k < XMM_SLOTS; ++k) {
        Slot &sl = m->slot[k];
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
        free_slot(sl);
        dfree(sl.d_state); dfree(sl.d_keys); dfree(sl.d_summary); hfree(sl.h_summary);
        for (int i = 0; i < 3; ++i)
            if (sl.ev[i]) (void)hipEventDestroy(sl.ev[i]);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
    }
    delete m;
    return XM_OK;
}

int xm_mapp_reserve(xm_mapp *m, int slot, uint64_t window_bytes, uint64_t max_lines, uint64_t max_values)
{
    if (bad_slot(m, slot) || window_bytes > XMM_MAX_WINDOW || max_lines == 0 || max_lines >= 0xFFFFFF00ull || max_values > XMM_MAX_WINDOW)
        return XM_ERR_INVALID_ARG;
    XMF_HIP(m, hipSetDevice(m->device));
    Slot &sl = m->slot[slot];
    XMF_HIP(m, hipStreamSynchronize(sl.stream));
    // a window begins here: whatever an abandoned one had sent is forgotten
    sl.uploaded = 0;
    sl.marked = 0;
    sl.state_cleared = false;
    sl.upload_timed = false;
    sl.window = sl.max_lines = sl.max_values = 0;
    // a failed growth leaves the capacity at 0 and the pointers freed or null: the next reserve allocates afresh
    XMF_TRY(grow_window(m, sl, std::max<uint64_t>(window_bytes, 1)));
    XMF_TRY(grow_lines(m, sl, max_lines));
    XMF_TRY(grow_values(m, sl, max_values));
    sl.window = std::max<uint64_t>(window_bytes, 1);
    sl.max_lines = max_lines;
    sl.max_values = max_values;
    return XM_OK;
}

char *xm_mapp_staging(xm_mapp *m, int slot)
{
    if (bad_slot(m, slot)) return nullptr;
    return m->slot[slot].h_text;
}

int xm_mapp_upload(xm_mapp *m, int slot, uint64_t offset, uint64_t bytes)
{
    if (bad_slot(m, slot)) return XM_ERR_INVALID_ARG;
    Slot &sl = m->slot[slot];
    if (offset == 0) { sl.uploaded = 0; sl.marked = 0; sl.state_cleared = false; }      // a new window (the one before may have been abandoned)
    if (sl.max_lines == 0 || offset != sl.uploaded || offset + bytes > sl.window) return XM_ERR_INVALID_ARG;
    if (bytes == 0) return XM_OK;
    XMF_HIP(m, hipSetDevice(m->device));
    if (!sl.upload_timed) {
        XMF_HIP(m, hipEventRecord(sl.ev[0], sl.stream));
        sl.upload_timed = true;
    }
    // M1 on the chunks that are complete (the window's last chunk needs the window's true length: xm_mapp_run marks what is left)
    XMF_TRY(mark_chunks(m, sl, offset + bytes, (uint32_t)((offset + bytes) / xmm::CHUNK)));
    XMF_HIP(m, hipGetLastError());
    sl.uploaded = offset + bytes;
    return XM_OK;
}

int xm_mapp_run(xm_mapp *m, int slot, uint64_t len, int eof, const uint8_t *carry_key, uint32_t carry_key_len, int has_carry,
                uint32_t carry_position, xm_mapp_block *out)
{
    if (bad_slot(m, slot) || !out || (has_carry && carry_key_len && !carry_key)) return XM_ERR_INVALID_ARG;
    Slot &sl = m->slot[slot];
    const uint64_t sent = sl.uploaded;
    const bool timed = sl.upload_timed;
    sl.uploaded = 0;
    sl.upload_timed = false;
    if (sl.max_lines == 0 || len > sl.window || sent > len) {
        sl.marked = 0;
        sl.state_cleared = false;
        return XM_ERR_INVALID_ARG;
    }
    XMF_HIP(m, hipSetDevice(m->device));
    hipStream_t st = sl.stream;
    if (sent == 0) { sl.marked = 0; sl.state_cleared = false; }     // nothing of this window was announced: all of it is marked here
    const uint32_t klen = has_carry ? carry_key_len : 0u;
    if (klen > sl.key_cap) {
        XMF_HIP(m, hipStreamSynchronize(st));
        sl.key_cap = 0;
        XMF_TRY(dalloc(m, sl.d_key, (size_t)klen + 64));
        sl.key_cap = (uint64_t)klen + 64;
    }

    xmm::Job job;
    std::memset(&job, 0, sizeof job);
    job.text = sl.d_text;
    job.len = (uint32_t)len;
    job.eof = eof ? 1u : 0u;
    job.n_chunks = (uint32_t)((len + xmm::CHUNK - 1) / xmm::CHUNK);
    job.mask16 = sl.d_mask; job.chunk_cnt = sl.d_chunk_cnt; job.chunk_base = sl.d_chunk_base;
    job.cap_lines = (uint32_t)sl.max_lines;
    job.lend = sl.d_lend; job.np = sl.d_np; job.tlen = sl.d_tlen; job.roff = sl.d_roff; job.rlen = sl.d_rlen; job.seg_of = sl.d_seg_of;
    job.flags = sl.d_flags;
    job.part = sl.d_part; job.part_base = sl.d_part_base; job.vpart = sl.d_vpart; job.vbase = sl.d_vbase;
    job.segs = sl.d_segs;
    job.values = sl.d_values;
    job.max_values = sl.max_values;
    job.state = sl.d_state; job.keys = sl.d_keys; job.summary = sl.d_summary;
    job.carry_key = sl.d_key;
    job.carry_key_len = klen;
    job.has_carry = has_carry ? 1u : 0u;
    job.carry_position = has_carry ? carry_position : 0u;

    if (!timed) XMF_HIP(m, hipEventRecord(sl.ev[0], st));
    int rc = mark_chunks(m, sl, len, job.n_chunks);              // that is where the text crosses the link
    sl.marked = 0;
    sl.state_cleared = false;
    if (rc != XM_OK) return rc;
    XMF_HIP(m, hipEventRecord(sl.ev[1], st));
    if (klen) XMF_HIP(m, hipMemcpyAsync(sl.d_key, carry_key, klen, hipMemcpyHostToDevice, st));
    xmm::enqueue_behind_mark(job, st);
    XMF_HIP(m, hipGetLastError());
    XMF_HIP(m, hipEventRecord(sl.ev[2], st));
    XMF_HIP(m, hipMemcpyAsync(sl.h_summary, sl.d_summary, xmm::SUM_WORDS * sizeof(xmm::u64), hipMemcpyDeviceToHost, st));
    XMF_HIP(m, hipStreamSynchronize(st));

    const xmm::u64 *sum = sl.h_summary;
    std::memset(out, 0, sizeof *out);
    out->consumed = sum[xmm::SUM_CONSUMED];
    out->n_lines = sum[xmm::SUM_NLINES];
    out->n_segments = sum[xmm::SUM_NSEG];
    out->n_values = sum[xmm::SUM_NVALUES];
    out->status = (int32_t)sum[xmm::SUM_STATUS];
    out->reason = (int32_t)sum[xmm::SUM_REASON];
    out->declined_line = sum[xmm::SUM_DECLINED];
    out->carry_position = (uint32_t)sum[xmm::SUM_CARRY_POS];
    out->carry_settled = (int32_t)sum[xmm::SUM_CARRY_SETTLED];
    if (out->n_segments > sl.max_lines || out->n_values > sl.max_values) return XM_ERR_HIP;        // never: the kernels' own limits
    if (out->n_segments) XMF_HIP(m, hipMemcpyAsync(sl.h_segs, sl.d_segs, out->n_segments * sizeof(xmm::Seg), hipMemcpyDeviceToHost, st));
    if (out->n_values) XMF_HIP(m, hipMemcpyAsync(sl.h_values, sl.d_values, out->n_values, hipMemcpyDeviceToHost, st));
    if (out->n_segments || out->n_values) XMF_HIP(m, hipStreamSynchronize(st));
    out->segments = reinterpret_cast<const xm_mapp_segment *>(sl.h_segs);
    out->values = sl.h_values;
    (void)hipEventElapsedTime(&out->ms_upload, sl.ev[0], sl.ev[1]);
    (void)hipEventElapsedTime(&out->ms_kernels, sl.ev[1], sl.ev[2]);
    return XM_OK;
}

const char *xm_mapp_last_error(const xm_mapp *m) { return last_error_text(m); }

}  // extern "C"
