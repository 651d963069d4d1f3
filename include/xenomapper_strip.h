/*
 * xenomapper_strip.h -- C ABI of the SAM column stripper that runs ON the GPU (libxenomapper_hip.so, gfx950).
 *
 * The reference reads its two SAM files line by line on one core -- getReadPairs
 * (/root/reference/xenomapper/xenomapper.py:95-118: readline, strip, split, compare the names) and the text half
 * of tag_func (get_tag :176-191, get_tag_with_ZS_as_XS :193-206: find the optional fields that contain "AS" /
 * "XS" / "ZS", int() of what follows the last ':').  include/xenomapper_host.h does that with host threads
 * (xmh_parse); this header is the same step with the text shipped to the device instead: the host only copies
 * the two windows of text into page-locked staging buffers, the kernels index the lines (universal newlines),
 * split them by Python's white space rules, find the tags, compare the names and leave the score columns and
 * the unit mask IN HBM, where the classify kernels (include/xenomapper_hip.h) read them -- no column ever
 * crosses PCIe.  What comes back is what the line writer (xmh_emit) needs: where every line starts and ends.
 *
 * Same exactness contract as xmh_parse: a value that is not a plain int32 integer or a tag that matches twice
 * is flagged per line (XMS_LINE_EX_*), never guessed; non-ASCII input is refused as a whole (non_ascii).  The
 * caller resolves flagged records with the reference-equivalent text functions (xm_strip_columns brings the
 * columns to the host for that) or hands the window to xmh_parse.
 *
 * Scope: SAM text, all three built-in plugins, the walk with and without --skip_repeated_reads (xenomapper.py:110-117).
 * Windows are shorter than 4 GiB - 64 KiB.  BAM input, windows beyond that and non-ASCII text stay with xenomapper_host.h.
 * The six outputs come back as text (xm_strip_fetch_bins) or as BAM: every wanted line encoded as a BAM alignment record on the
 * device, in BGZF members of stored blocks (xm_strip_fetch_bins_bam) or of deflated ones (xm_strip_fetch_bins_bamz).  The BAM header
 * made from the @SQ lines is the caller's, who also supplies the reference names (xm_strip_set_refs); the file path behind
 * classify_sam_files(encode_sam=True) does both and sends the windows the device declines through xmh_sam_encode.
 *
 * A stripper has two slots so that one window pair can be copied, uploaded and stripped (one host thread) while
 * the block before it is classified and written (another thread); calls on one slot must not overlap.
 */
#ifndef XENOMAPPER_STRIP_H
#define XENOMAPPER_STRIP_H

#include "xenomapper_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XMS_ABI_VERSION 4   /* 2: xm_strip_fetch_bins / xm_strip_out_wait.  3: two calls for reading a window ahead (begun behind
                               a gap, its lead set later).  4: those two withdrawn -- reading ahead measured no better.  Additive since,
                               the version unchanged: xm_strip_set_refs / xm_strip_fetch_bins_bam, then xm_strip_fetch_bins_bamz */
#define XMS_SLOTS 2
#define XMS_MAX_WINDOW 0xFFFF0000ull

/* score_mode (the values of XMH_SCORE_*) */
#define XMS_SCORE_AS_XS 0   /* get_tag                 xenomapper.py:176-191 */
#define XMS_SCORE_AS_ZS 1   /* get_tag_with_ZS_as_XS   xenomapper.py:193-206 */
#define XMS_SCORE_CIGAR 2   /* get_cigarbased_AS_tag   xenomapper.py:228-256: NM + the CIGAR operations, as the packed CIGAR columns of
                               xenomapper_hip.h, left on the device; XS by get_tag */

/* line flags; bit 0 is XMH_LINE_NORMAL of xenomapper_host.h */
#define XMS_LINE_NORMAL   0x01u  /* the line already equals '\t'.join(fields)                                     */
#define XMS_LINE_BLANK    0x02u  /* no field at all: ends the walk (xenomapper.py:105)                            */
#define XMS_LINE_EX_A     0x1Cu  /* bits 2-4: exception kind of the AS column (XMH_EX_*: 1 NONINT, 2 DUP; CIGAR mode, about NM and
                                    the CIGAR field: 1 NONINT, 3 SHORT, 4 BIGLEN), 0 = none                           */
#define XMS_LINE_EX_A_SHIFT 2
#define XMS_LINE_EX_X     0x60u  /* bits 5-6: same for the XS (or ZS) column: 0, 1, 2                                */
#define XMS_LINE_EX_X_SHIFT 5
#define XMS_LINE_MISMATCH 0x80u  /* file-1 flags only: the names of the two files differ (xenomapper.py:106)      */

typedef struct xm_strip xm_strip;

/* Result of xm_strip_run; the fields up to mismatch_at mean what they mean in xmh_block.  The arrays are page-locked
 * host memory owned by the stripper: n_records entries each, valid until the next xm_strip_run on the same slot. */
typedef struct {
    uint64_t n_records;
    uint64_t consumed1, consumed2;
    uint64_t consumed_lines1, consumed_lines2;
    int32_t  ended, starved;
    int64_t  mismatch_at;
    int32_t  non_ascii;        /* 1: a byte >= 0x80 in either window; nothing else of the result is meaningful */
    int32_t  overflow;         /* 1: the skipping walk met more lines than max_records + 1 in a window (or the packed CIGAR
                                  operations outgrew their array): nothing else is meaningful, strip the window with xmh_parse */
    uint64_t n_exceptions;     /* records among the n_records whose flags carry XMS_LINE_EX_A / _EX_X on either line */
    uint64_t n_lines1, n_lines2;                        /* lines found in each window (complete ones; the last one of a file too) */
    const uint32_t *line_off1, *line_off2;              /* first byte of the record's line in its window */
    const uint32_t *line_len1, *line_len2;              /* bytes without the terminator */
    const uint32_t *norm_len1, *norm_len2;              /* length of '\t'.join(fields) */
    const uint8_t  *line_flags1, *line_flags2;          /* XMS_LINE_* */
    float ms_upload, ms_kernels;                        /* device time from the first upload to the last, and of the kernels (HIP events) */
} xm_strip_block;

int xms_abi_version(void);

/* ctx: the classifier context the columns will be classified with (same device).  Allocates nothing large. */
int xm_strip_create(xm_ctx *ctx, int device_id, xm_strip **out);
int xm_strip_destroy(xm_strip *s);      /* while ctx is still alive: the slot streams are handed back to it (xm_workspace_release) */

/* Make the slot's buffers hold windows of window_bytes per file and max_records records (grows only; not to be called
 * while the slot is in use).  XM_ERR_INVALID_ARG beyond XMS_MAX_WINDOW. */
int xm_strip_reserve(xm_strip *s, int slot, uint64_t window_bytes, uint64_t max_records);

/* Page-locked staging buffer of a slot for file 0 / 1 (window_bytes long): the caller copies the window there. */
char *xm_strip_staging(xm_strip *s, int slot, int file);

/* Start the upload of bytes [offset, offset + bytes) of a staged window (asynchronous, on the slot's stream): called piece by
 * piece, in order from offset 0, while the host is still copying the rest of the window into the staging buffer, it hides
 * the copy behind the PCIe transfer.  The bytes cross the link inside the first kernel, which reads the staging buffer itself
 * and writes the window's copy in HBM (no copy engine launch per piece).  Optional: xm_strip_run uploads whatever has not been
 * sent. */
int xm_strip_upload(xm_strip *s, int slot, int file, uint64_t offset, uint64_t bytes);

/*
 * Upload the two staged windows (len1 / len2 bytes; eof*: the window reaches the end of its file) and strip them.
 * paired: the unit mask is name[k] == name[k-1] (else every record is a unit); skip_repeated / keep_halo / max_records as
 * in xmh_parse.  Blocking (the slot's own stream).  The columns of the block stay on the device for xm_strip_classify.
 */
int xm_strip_run(xm_strip *s, int slot, uint64_t len1, int eof1, uint64_t len2, int eof2,
                 int score_mode, int paired, int skip_repeated, int keep_halo, uint64_t max_records, xm_strip_block *out);

/*
 * The fused main loop (xm_classify_compact_dev; after a XMS_SCORE_CIGAR run xm_classify_compact_cigar_packed_dev, with
 * XM_ERR_RANGE when a synthesised score leaves int32) on the first n_records records of the slot's block.  Results in
 * page-locked host arrays owned by the stripper, valid until the next call on the slot: code (n_records bytes), the six
 * index lists back to back (*idx) with bin_offsets[8], counts[64].
 */
int xm_strip_classify(xm_strip *s, int slot, int mode, uint64_t n_records, int32_t min_score_floor,
                      const uint8_t **code, const uint32_t **idx, uint64_t bin_offsets[8], uint64_t counts[64]);

/*
 * After xm_strip_classify: the six OUTPUTS themselves, gathered on the device (ABI 2) -- for every bin whose sink is given
 * (sink_mask bit b) the lines the reference's loop prints for the bin's units, in input order (xenomapper.py:332-350, :423-448,
 * :521-550: primary bins file 1's line(s), secondary bins file 2's, `unresolved` file 1's then file 2's; a paired unit is
 * records i - 1 and i), each as '\t'.join(fields) + '\n'.  One page-locked stream owned by the stripper, valid after
 * xm_strip_out_wait and until the next call on the slot: bin b's text = text[bin_off[b] .. bin_off[b + 1]), b = 0..5 in the state
 * order PS, SS, PM, SM, unresolved, unassigned.  The copy to the host runs on a stream of the slot's own, beside the next
 * window's upload and kernels.  status 0: on its way; 2: more text than the buffers hold (units that overlap); 3: a wanted
 * line is not '\t'.join(fields) as it stands (mixed white space) -- then nothing was copied: write this window with xmh_emit
 * from the line tables of xm_strip_run.
 */
typedef struct {
    const uint8_t *text;
    uint64_t bin_off[8];
    int32_t  status, reserved;
} xm_strip_bins;
int xm_strip_fetch_bins(xm_strip *s, int slot, uint64_t n_records, int paired, uint32_t sink_mask, xm_strip_bins *out);
int xm_strip_out_wait(xm_strip *s, int slot);      /* blocks until the stream asked for last has arrived (any thread) */

/*
 * The six outputs as BAM.  xm_strip_set_refs: the reference names of file 0 / 1, as xm_bamdev_set_refs takes them (the names back
 * to back, at[n_refs + 1] positions), once per file and for both slots; an open-addressed table of them is built on the host and
 * uploaded (XM_ERR_INVALID_ARG: a name twice).  Not to be called while a slot is in use.
 * xm_strip_fetch_bins_bam, after xm_strip_classify, is xm_strip_fetch_bins with every wanted line encoded as the BAM alignment record
 * htslib's SAM parser writes for it (the rule: csrc/xm_samrec.h; xmh_sam_encode of xenomapper_host.h is the same rule on the host)
 * and the records framed as xm_bamdev_fetch_bins_bam frames them: bin b's bytes = text[bin_off[b] .. bin_off[b + 1]), a whole number
 * of complete BGZF members of one stored block each, none when the bin has no wanted unit; every member but a bin's last holds
 * block_payload record bytes (64 .. 65280; 0 = 65280), so a record may span members.  ref_shift is added to refID and next_refID of
 * file 2's records in bin 4 where they are >= 0.  The caller puts a BAM header in front and the end-of-file member behind.
 * status 0: on its way (xm_strip_out_wait).  Otherwise nothing was copied, and the window is the host's (xmh_sam_encode):
 *   1: a wanted line the device does not encode -- reason = XMS_ENC_*, declined_record / declined_file (0, 1) = the first such line
 *      in the order of the output; a host-only form (XMS_ENC_HOST_*: an f or B:f field, more than 65535 CIGAR operations, a SEQ byte
 *      outside the 16 upper-case codes, a number that is not canonical) or a line outside the grammar, which the host reports
 *   2: more bytes than the slot's buffers hold
 *   3: a wanted line that is not XMS_LINE_NORMAL (looked at before 1)
 * Only wanted lines decide.  XM_ERR_INVALID_ARG without the references of a file whose lines are wanted.  The call shares the slot's
 * output stream with xm_strip_fetch_bins: either may follow the other on one classified block.
 */
#define XMS_ENC_FIELDS          1   /* fewer than 11 fields */
#define XMS_ENC_QNAME           2   /* not 1 - 254 bytes */
#define XMS_ENC_FLAG            3
#define XMS_ENC_RNAME           4   /* not '*' and not in the reference list */
#define XMS_ENC_POS             5
#define XMS_ENC_MAPQ            6
#define XMS_ENC_CIGAR           7
#define XMS_ENC_RNEXT           8
#define XMS_ENC_PNEXT           9
#define XMS_ENC_TLEN            10
#define XMS_ENC_SEQ             11
#define XMS_ENC_QUAL            12  /* not '*' and not l_seq bytes in '!' - '~' */
#define XMS_ENC_AUX             13  /* an optional field that is not TG:T:V of a known type */
#define XMS_ENC_AUX_RANGE       14  /* a value outside its type's range */
#define XMS_ENC_SIZE            15
#define XMS_ENC_HOST_FLOAT      32
#define XMS_ENC_HOST_LONG_CIGAR 33
#define XMS_ENC_HOST_SEQ_CODE   34
#define XMS_ENC_HOST_NUMBER     35
int xm_strip_set_refs(xm_strip *s, int file, const uint8_t *names, const uint32_t *at, uint32_t n_refs);
typedef struct {
    const uint8_t *text;
    uint64_t bin_off[8];
    int32_t  status, reason;
    uint64_t declined_record;
    int32_t  declined_file, reserved;
} xm_strip_bam_bins;
int xm_strip_fetch_bins_bam(xm_strip *s, int slot, uint64_t n_records, int paired, uint32_t sink_mask, uint32_t block_payload,
                            int32_t ref_shift, xm_strip_bam_bins *out);
/*
 * The same six outputs as ordinary, COMPRESSED BAM: arguments, result, records and their order per bin as xm_strip_fetch_bins_bam,
 * status / reason / declined_* decided by the same rules at the same points, but every member holds what xm_bgzf_deflate_dev makes
 * of its payload (xenomapper_bgzf.h).  Bin b's bytes = text[bin_off[b] .. bin_off[b + 1]) are exactly those of xm_bgzf_compress on the
 * bin's records at block_payload, member for member; a bin without wanted units gets no member.  status 2 is decided by the stored
 * call's sums (payload + 31 per member), which a deflated member never exceeds.  The call waits for the encoder -- the members'
 * places are the scan of their lengths --: bin_off is final when it returns.  A member the encoder declines is XM_ERR_HIP
 * (xm_strip_last_error).  The slot's first such call makes what only this route needs -- a place per member's stream, three words
 * per member and the encoder's scratch (xm_bgzf_deflate_work_bytes()) --: XM_ERR_OOM when they cannot be made; xm_strip_destroy
 * frees them.  xm_strip_fetch_bins_bam and xm_strip_fetch_bins may still follow on the same classified block, in either order.
 */
int xm_strip_fetch_bins_bamz(xm_strip *s, int slot, uint64_t n_records, int paired, uint32_t sink_mask, uint32_t block_payload,
                             int32_t ref_shift, xm_strip_bam_bins *out);

/* Bring the first n_records of the slot's score columns and ceil(n/64) words of the unit mask to the host (for records
 * the caller must patch by the text rules).  Any pointer may be NULL. */
int xm_strip_columns(xm_strip *s, int slot, uint64_t n_records, int32_t *as1, int32_t *xs1, int32_t *as2, int32_t *xs2,
                     uint64_t *unit_bits);

/* After a XMS_SCORE_CIGAR run: the packed CIGAR columns of one file for the first n_records records copied to the host (any
 * pointer may be NULL; cig_tile: XM_CIG_TILES(n_records) + 1 words; *n_ops = words of cig_ops in use).  For tests and for
 * callers that want the columns themselves. */
int xm_strip_cigar_columns(xm_strip *s, int slot, int file, uint64_t n_records, int32_t *nm, uint8_t *cig_cnt, uint32_t *cig_tile,
                           uint32_t *cig_ops, uint64_t ops_capacity, uint64_t *n_ops);

/* Device addresses of the slot's columns: as1, xs1, as2, xs2 (int32) and unit_bits (uint64), for callers that launch the
 * classify kernels themselves (xm_classify_*_dev). */
int xm_strip_device_columns(xm_strip *s, int slot, void *ptrs[5]);

/* Text of the last failing HIP call of this stripper (empty string if none). */
const char *xm_strip_last_error(const xm_strip *s);

#ifdef __cplusplus
}
#endif
#endif /* XENOMAPPER_STRIP_H */
