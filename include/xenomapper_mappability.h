/*
 * xenomapper_mappability.h -- C ABI of the single-end mappability step that runs ON the GPU (libxenomapper_hip.so, gfx950).
 *
 * The reference's xenomappability tool turns the name-sorted SAM of one simulated read per genome position into a 0/1 track
 * per chromosome (xenomapper/mappability.py:175-214, single_end_mappability_from_sam): one Python loop over every line.  Here
 * the host only reads windows of the text into a page-locked staging buffer; the kernels index the lines, parse the five
 * fields that matter, find where the loop would begin a new track (a two-state automaton over three booleans per line, resolved
 * by a prefix scan) and scatter one byte per line.  What comes back is a table of segments and their values.
 *
 * The loop's state is (cur, position, values).  A window is run with the state carried in: has_carry (cur is set), carry_key
 * (cur) and carry_position.  A segment is a stretch of lines that belong to one track: the first may continue the carried one
 * (starts 0, key_len 0: base = carry_position); every other begins a track under key = RNAME of its first line, with
 * base = name_pos of that line - 1 implied zeros in front.  A segment's values are those of positions base + 1 .. last_pos.
 *
 * The device takes this grammar only; anything else declines the whole window (status XMM_DECLINED, the reason and the first
 * offending line), and the caller runs the reference's loop on window[0, consumed):
 *   - lines end with '\n' only (the last line of the file may lack it); ASCII; no str.split() separator but '\t' and '\n'
 *   - at least 11 tab-separated fields, none of the first 11 empty
 *   - the name's part behind its last '_' (the whole name without one) and POS: 1 - 10 ASCII digits, at most 2^32 - 1
 *   - MAPQ is compared with the two bytes "42"; RNAME and the name's part in front of its last '_' as bytes
 *   - name_pos increases strictly inside a segment, is above carry_position in the carried one and is never 0
 * Of several reasons the one of the first line counts; inside one line a byte reason goes before a field reason.
 *
 * One or two slots; calls on one slot must not overlap.  The front end never touches the context's compaction workspace.
 */
#ifndef XENOMAPPER_MAPPABILITY_H
#define XENOMAPPER_MAPPABILITY_H

#include "xenomapper_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XMM_ABI_VERSION 1
#define XMM_SLOTS 2
#define XMM_MAX_WINDOW 0xFFFF0000ull

/* status */
enum { XMM_OK_WINDOW = 0, XMM_DECLINED = 1, XMM_TOO_MANY_LINES = 2, XMM_TOO_MANY_VALUES = 3 };
/* reason */
enum {
    XMM_R_NONE = 0,
    XMM_R_NON_ASCII = 1,      /* a byte >= 0x80 */
    XMM_R_SEPARATOR = 2,      /* '\r', ' ', 0x0B, 0x0C, 0x1C - 0x1F */
    XMM_R_FIELDS = 3,         /* fewer than 11 fields, or an empty one among the first 11 */
    XMM_R_NAME_NUMBER = 4,
    XMM_R_POS_NUMBER = 5,
    XMM_R_NOT_SEQUENTIAL = 6
};

typedef struct xm_mapp xm_mapp;

typedef struct {
    uint32_t first_line, n_lines;
    uint32_t key_off, key_len;   /* RNAME of the first line, in the window; key_len 0 and starts 0: the segment carried in */
    uint32_t starts;
    uint32_t base, last_pos;
    uint32_t reserved;
    uint64_t value_off, n_values;
} xm_mapp_segment;

typedef struct {
    uint64_t consumed, n_lines, n_segments, n_values;   /* consumed: behind the last '\n', or the window's end when eof */
    int32_t  status, reason;
    uint64_t declined_line;
    const xm_mapp_segment *segments;
    const uint8_t *values;       /* page-locked, valid until the next run on the slot */
    uint32_t carry_position;     /* the state behind the window (status 0; else what was carried in) */
    int32_t  carry_settled;
    float    ms_upload, ms_kernels;
} xm_mapp_block;

int xmm_abi_version(void);

int xm_mapp_create(xm_ctx *ctx, int device_id, xm_mapp **out);
int xm_mapp_destroy(xm_mapp *m);

/* Make the slot's buffers hold a window of window_bytes, max_lines lines and max_values values (grows only; not while the slot
 * is in use).  XM_ERR_INVALID_ARG beyond XMM_MAX_WINDOW, for max_lines 0 or above 2^32 - 256, for max_values above XMM_MAX_WINDOW. */
int xm_mapp_reserve(xm_mapp *m, int slot, uint64_t window_bytes, uint64_t max_lines, uint64_t max_values);

/* Page-locked staging buffer of a slot (window_bytes long): the caller reads the window into it. */
char *xm_mapp_staging(xm_mapp *m, int slot);

/* Optional, piece by piece in order from offset 0, as xm_strip_upload: the bytes cross the link inside the first kernel. */
int xm_mapp_upload(xm_mapp *m, int slot, uint64_t offset, uint64_t bytes);

/* The staged window of len bytes (eof: it reaches the end of the file) with the carried state.  window_bytes, max_lines and
 * max_values are those of the slot's LAST reserve, whatever the buffers have grown to: XM_ERR_INVALID_ARG for a len (or an upload)
 * beyond that window_bytes, and on a slot never reserved.  Blocking (the slot's own stream). */
int xm_mapp_run(xm_mapp *m, int slot, uint64_t len, int eof, const uint8_t *carry_key, uint32_t carry_key_len, int has_carry,
                uint32_t carry_position, xm_mapp_block *out);

const char *xm_mapp_last_error(const xm_mapp *m);

#ifdef __cplusplus
}
#endif
#endif /* XENOMAPPER_MAPPABILITY_H */
