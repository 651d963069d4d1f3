// xm_samenc.cpp -- xmh_sam_encode (include/xenomapper_host.h): SAM lines to BAM alignment records on the host, with xm_samrec.h's
// rule in its HOST form: what the device encoder (xm_strip.hip, E1 / E2) is checked against, and the route for the windows it declines.
#include "../../include/xenomapper_host.h"

#include <new>
#include <vector>

#include "xm_samrec.h"

static_assert(XMH_ENC_FIELDS == xmsam::ENC_FIELDS && XMH_ENC_QNAME == xmsam::ENC_QNAME && XMH_ENC_FLAG == xmsam::ENC_FLAG &&
              XMH_ENC_RNAME == xmsam::ENC_RNAME && XMH_ENC_POS == xmsam::ENC_POS && XMH_ENC_MAPQ == xmsam::ENC_MAPQ &&
              XMH_ENC_CIGAR == xmsam::ENC_CIGAR && XMH_ENC_RNEXT == xmsam::ENC_RNEXT && XMH_ENC_PNEXT == xmsam::ENC_PNEXT &&
              XMH_ENC_TLEN == xmsam::ENC_TLEN && XMH_ENC_SEQ == xmsam::ENC_SEQ && XMH_ENC_QUAL == xmsam::ENC_QUAL &&
              XMH_ENC_AUX == xmsam::ENC_AUX && XMH_ENC_AUX_RANGE == xmsam::ENC_AUX_RANGE && XMH_ENC_SIZE == xmsam::ENC_SIZE &&
              XMH_ENC_HOST_FLOAT == xmsam::ENC_HOST_FLOAT && XMH_ENC_HOST_LONG_CIGAR == xmsam::ENC_HOST_LONG_CIGAR &&
              XMH_ENC_HOST_SEQ_CODE == xmsam::ENC_HOST_SEQ_CODE && XMH_ENC_HOST_NUMBER == xmsam::ENC_HOST_NUMBER,
              "the reason codes of xenomapper_host.h are xm_samrec.h's");

extern "C" int xmh_sam_encode(const uint8_t *text, const uint64_t *line_off, const uint32_t *line_len, uint64_t n, const uint8_t *names,
                              const uint32_t *at, uint32_t n_refs, int32_t ref_shift, int device_forms, uint8_t *out, uint64_t out_cap,
                              uint32_t *sizes, uint64_t *out_len, uint64_t *bad_line, int32_t *reason)
{
    if (!out_len || !bad_line || !reason || (n && (!text || !line_off || !line_len)) || (n_refs && (!names || !at)))
        return XMH_ERR_INVALID_ARG;
    *out_len = 0;
    *bad_line = ~0ull;
    *reason = 0;
    for (uint32_t k = 0; k < n_refs; ++k)
        if (at[k + 1] < at[k]) return XMH_ERR_INVALID_ARG;
    std::vector<uint32_t> table;
    uint32_t mask = 0;
    try {
        if (!xmsam::build_ref_table(names, at, n_refs, table, mask)) return XMH_ERR_INVALID_ARG;      // a name twice
    } catch (const std::bad_alloc &) {
        return XMH_ERR_OOM;
    }
    const xmsam::RefHash refs{names, at, table.data(), mask, n_refs};
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t *line = text + line_off[i];
        const xmsam::Sized sz = device_forms ? xmsam::size_of<false>(line, line_len[i], refs) : xmsam::size_of<true>(line, line_len[i], refs);
        if (sz.reason != xmsam::ENC_OK) {                 // the line and the reason; nothing of it or behind it is encoded
            *bad_line = i;
            *reason = sz.reason;
            break;
        }
        if (sizes) sizes[i] = sz.size;
        if (out) {
            if (total + sz.size > out_cap) return XMH_ERR_INVALID_ARG;
            const int32_t rc = device_forms ? xmsam::write<false>(line, line_len[i], refs, ref_shift, sz, out + total, nullptr)
                                            : xmsam::write<true>(line, line_len[i], refs, ref_shift, sz, out + total, nullptr);
            if (rc != xmsam::ENC_OK) return XMH_ERR_INVALID_ARG;
        }
        total += sz.size;
    }
    *out_len = total;
    return XMH_OK;
}
