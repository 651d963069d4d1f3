// xm_mapp_kernels.h -- the device code of the single-end mappability front end (C ABI: include/xenomapper_mappability.h; host
// half: xm_mapp.hip).  Device code and its launch sequence only, so that tests/lockstep_mapp_host.cpp can compile it as plain
// C++ through the lockstep shim and run every launch lane by lane.
//
// What is computed is the loop of single_end_mappability_from_sam (xenomapper_amd/mappability.py; the reference's
// xenomapper/mappability.py:175-214) on one window of name-sorted SAM text, with the state the loop carries in:
//   M1  mark_kernel       16 bytes a lane, read from the page-locked staging buffer over the link and written to the HBM copy:
//                         '\n' bits per 16-byte group, '\n' per wave quarter of a 64 KiB chunk, the first byte >= 0x80, the first
//                         str.split() separator other than '\t' and '\n', the end of the last '\n'
//   M2  chunk_scan_kernel exclusive scan of the counts; lines, consumed bytes, too many lines
//   M3  fill_kernel       lend[i] = where line i's '\n' is
//   M4  parse_kernel      one lane per line: the first five fields and the 11-field rule -> name_pos, value bit, g, the T and RNAME
//                         spans, a decline reason (first declined line by atomicMin)
//   M5a relate_kernel     e, x of every line against the line in front (line 0: against the carried key); a tile's 256 two-bit
//                         maps composed into one
//   M5b map_part_kernel   scan of the tiles' maps
//   M5c start_kernel      the maps scanned inside the tile -> every line's incoming state -> start flag; not-sequential test (first
//                         by atomicMin); starts per tile
//   M5d cnt_part_kernel   scan of the tiles' start counts; the number of segments
//   M5e seg_kernel        segment id per line; a segment's first line writes its table row
//   M5f segfin_kernel     one lane per segment: lines, last name_pos, n_values; n_values per tile of segments
//   M5g val_part_kernel   scan of those (64 bits); then one lane decides the window: status, reason, first declined line, carry
//   M5h segoff_kernel     value_off of every segment
//   M6  zero_kernel, scatter_kernel   the values buffer cleared as far as used; one byte per line
// A line's map takes the state in front of it (0 settled: cur == T of the line in front; 1 unsettled: the line in front started a
// segment under an RNAME that is not its T) to the state behind it.  Two bits: bit s = the state behind for state s in front.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifdef XM_LOCKSTEP_HOST
#define XMM_LAUNCH(kernel, grid, block, st, ...) do { (void)(st); ls::launch(grid, block, [&] { kernel(__VA_ARGS__); }); } while (0)
#else
#define XMM_LAUNCH(kernel, grid, block, st, ...) kernel<<<grid, block, 0, st>>>(__VA_ARGS__)
#endif

namespace xmm {

typedef unsigned long long u64;

constexpr int MB = 256;                               // lanes per workgroup, lines (or segments) per tile
constexpr uint32_t CHUNK = 1u << 16;                  // bytes of text per workgroup in M1 / M3
constexpr uint32_t GROUPS = CHUNK / 16;
constexpr uint32_t WAVES = MB / 64;
constexpr uint32_t ITER = GROUPS / MB;
constexpr uint32_t TEXT_PAD = 64;                     // bytes readable behind a window (M1: 16-byte groups, M4: 8-byte words)
constexpr uint32_t MAX_GRID = 2048;                   // the kernels stride over their lines / tiles

// reason codes and status: include/xenomapper_mappability.h (xm_mapp.hip asserts that they are equal)
enum { R_NONE = 0, R_NON_ASCII = 1, R_SEPARATOR = 2, R_FIELDS = 3, R_NAME_NUMBER = 4, R_POS_NUMBER = 5, R_NOT_SEQUENTIAL = 6 };
enum { S_OK = 0, S_DECLINED = 1, S_TOO_MANY_LINES = 2, S_TOO_MANY_VALUES = 3 };

// line flags
enum { F_VALUE = 1, F_E = 2, F_X = 4, F_G = 8, F_START = 16 };

// state words (uint32), cleared in front of the window's first M1 launch
enum { ST_BAD_HI = 0,      // 0xFFFFFFFF - the offset of the first byte >= 0x80 (0: none), by atomicMax
       ST_BAD_SEP,         // the same for the first separator that is neither '\t' nor '\n'
       ST_LAST_LF,         // the offset behind the last '\n' (0: none)
       ST_NTERM,           // '\n' in the window
       ST_N,               // lines the kernels work on (0 when there are more than cap_lines)
       ST_NSEG, ST_STATUS, ST_SETTLED, ST_WORDS = 8 };
// 64-bit words
enum { K_GRAMMAR = 0,      // (line << 8 | reason) of the first line M4 declines, ~0: none
       K_NONSEQ,           // the first line that is not sequential, ~0: none
       K_NVALUES, K_WORDS = 4 };
enum { SUM_CONSUMED = 0, SUM_NLINES, SUM_NSEG, SUM_NVALUES, SUM_STATUS, SUM_REASON, SUM_DECLINED, SUM_CARRY_POS, SUM_CARRY_SETTLED,
       SUM_WORDS = 12 };

struct Seg {                                          // xm_mapp_segment
    uint32_t first_line, n_lines, key_off, key_len, starts, base, last_pos, pad_;
    u64 value_off, n_values;
};

struct Job {
    const uint8_t *text;                              // the window's copy in HBM
    uint32_t len, eof, n_chunks;
    uint16_t *mask16;
    uint32_t *chunk_cnt, *chunk_base;
    uint32_t cap_lines;                               // max_lines
    uint32_t *lend;                                   // cap_lines
    uint32_t *np, *tlen, *roff, *rlen, *seg_of;       // cap_lines each; a line's name begins where the line does
    uint8_t *flags;                                   // cap_lines
    uint32_t *part, *part_base;                       // per tile of lines: map, then start count; their scans
    u64 *vpart, *vbase;                               // per tile of segments
    Seg *segs;                                        // cap_lines
    uint8_t *values;
    u64 max_values;
    uint32_t *state;
    u64 *keys, *summary;
    const uint8_t *carry_key;
    uint32_t carry_key_len, has_carry, carry_position;
};

// what a slot's buffers hold for (window_bytes, max_lines, max_values): the front end allocates exactly these counts and the
// lockstep program does too
struct Sizes {
    size_t text, mask16, chunk_cnt, lines, tiles, values;
};
inline Sizes sizes_for(uint64_t window_bytes, uint64_t max_lines, uint64_t max_values)
{
    Sizes z;
    const uint64_t cap = (window_bytes + CHUNK - 1) / CHUNK * CHUNK;
    z.text = (size_t)cap + TEXT_PAD;
    z.mask16 = (size_t)(cap / 16);
    z.chunk_cnt = (size_t)(cap / CHUNK) * WAVES;
    z.lines = (size_t)max_lines;
    z.tiles = (size_t)((max_lines + MB - 1) / MB);
    z.values = (size_t)((max_values + 15) / 16 * 16);          // zero_kernel clears whole 16-byte words
    return z;
}

// ---- scans ------------------------------------------------------------------------------------------------------------------------
struct AddU32 {
    static __device__ __forceinline__ uint32_t id() { return 0u; }
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return a + b; }
};
struct AddU64 {
    static __device__ __forceinline__ u64 id() { return 0ull; }
    static __device__ __forceinline__ u64 op(u64 a, u64 b) { return a + b; }
};
struct Compose {                                      // a, then b
    static __device__ __forceinline__ uint32_t id() { return 2u; }
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b)
    {
        return ((b >> (a & 1u)) & 1u) | (((b >> ((a >> 1) & 1u)) & 1u) << 1);
    }
};

// Scan over the NW waves of a workgroup (ws: NW words of LDS, free again behind the call; two barriers).  Returns the fold of the
// lanes in front of this one (a composition has no inverse to take the lane's own value out of an inclusive scan with); incl: with
// this lane's; total: of all lanes.
template <typename T, typename Op, int NW>
__device__ __forceinline__ T block_scan(T v, T *ws, T &incl, T &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T in = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(in, o);
        if (lane >= o) in = Op::op(t, in);
    }
    const T up = __shfl_up(in, 1u);
    const T ex = lane ? up : Op::id();
    if (lane == 63u) ws[wave] = in;
    __syncthreads();
    T front = Op::id(), all = Op::id();
    for (uint32_t w = 0; w < (uint32_t)NW; ++w) {
        const T t = ws[w];
        if (w < wave) front = Op::op(front, t);
        all = Op::op(all, t);
    }
    __syncthreads();
    total = all;
    incl = Op::op(front, in);
    return Op::op(front, ex);
}

// exclusive scan of part[0, n) into base[0, n) by one workgroup of 1024 lanes; returns the total to every lane
template <typename T, typename Op>
__device__ __forceinline__ T part_scan(const T *part, T *base, uint32_t n, T *ws)
{
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t b = threadIdx.x * per < n ? threadIdx.x * per : n, e = b + per < n ? b + per : n;
    T sum = Op::id();
    for (uint32_t c = b; c < e; ++c) sum = Op::op(sum, part[c]);
    T incl, total;
    T run = block_scan<T, Op, 16>(sum, ws, incl, total);
    for (uint32_t c = b; c < e; ++c) {
        const T own = part[c];
        base[c] = run;
        run = Op::op(run, own);
    }
    return total;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- lines ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t line_start(const Job &j, uint32_t i) { return i ? j.lend[i - 1u] + 1u : 0u; }
__device__ __forceinline__ uint32_t line_end(const Job &j, uint32_t i, uint32_t n_terms) { return i < n_terms ? j.lend[i] : j.len; }

__device__ __forceinline__ bool span_equal(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb)
{
    if (na != nb) return false;
    for (uint32_t k = 0; k < na; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// text[b, e) as 1 - 10 ASCII digits with a value of at most 2^32 - 1
__device__ __forceinline__ bool plain_u32(const uint8_t *text, uint32_t b, uint32_t e, uint32_t &out)
{
    if (e <= b || e - b > 10u) return false;
    u64 v = 0;
    for (uint32_t p = b; p < e; ++p) {
        const uint32_t c = text[p];
        if (c < '0' || c > '9') return false;
        v = v * 10u + (u64)(c - '0');
    }
    if (v > 0xFFFFFFFFull) return false;
    out = (uint32_t)v;
    return true;
}

// ---- M1 ---------------------------------------------------------------------------------------------------------------------------
struct MarkArgs {
    const uint8_t *src;                               // the page-locked staging buffer
    uint8_t *copy;
    uint16_t *mask16;
    uint32_t *chunk_cnt, *state;
    uint32_t len, chunk0, n_chunks;                   // chunks [chunk0, chunk0 + n_chunks) of a window of `len` bytes
};

__global__ void __launch_bounds__(MB) mark_kernel(const MarkArgs a)
{
    const uint32_t chunk = a.chunk0 + blockIdx.x;
    const uint32_t n_groups = (a.len + 15u) / 16u;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t cnt = 0, bad_hi = 0, bad_sep = 0, last_lf = 0;       // bad_*: 0xFFFFFFFF - offset, 0 = none
    if (blockIdx.x < a.n_chunks) {
        for (uint32_t it = 0; it < ITER; ++it) {
            const uint32_t g = chunk * GROUPS + wave * (GROUPS / WAVES) + it * 64u + lane;
            if (g >= n_groups) break;
            const uint32_t p0 = g * 16u;
            const uint4 v = *reinterpret_cast<const uint4 *>(a.src + p0);         // the buffer is readable past len (TEXT_PAD)
            *reinterpret_cast<uint4 *>(a.copy + p0) = v;
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t lfm = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                // a byte below 0x21 or above 0x7F somewhere in the word?  ('\t' and '\n' are: nearly every other word of SAM text)
                const uint32_t x = w[q];
                const uint32_t low = (x - 0x21212121u) & ~x & 0x80808080u;
                if (((x & 0x80808080u) | low) == 0u) continue;
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t c = (x >> (8u * k)) & 0xFFu, p = p0 + 4u * q + k;
                    if (p >= a.len) break;
                    if (c == 10u) { lfm |= 1u << (4u * q + k); last_lf = p + 1u; }
                    else if (c >= 0x80u) { if (!bad_hi) bad_hi = 0xFFFFFFFFu - p; }
                    else if (c == 0x20u || (c >= 0x0Bu && c <= 0x0Du) || (c >= 0x1Cu && c <= 0x1Fu)) { if (!bad_sep) bad_sep = 0xFFFFFFFFu - p; }
                }
            }
            a.mask16[g] = (uint16_t)lfm;
            cnt += (uint32_t)__builtin_popcount(lfm);
        }
    }
    cnt = wave_sum(cnt);
    if (blockIdx.x < a.n_chunks && lane == 0u) a.chunk_cnt[chunk * WAVES + wave] = cnt;
    if (bad_hi) atomicMax(&a.state[ST_BAD_HI], bad_hi);
    if (bad_sep) atomicMax(&a.state[ST_BAD_SEP], bad_sep);
    if (last_lf) atomicMax(&a.state[ST_LAST_LF], last_lf);
}

// ---- M2 ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) chunk_scan_kernel(const Job job)
{
    __shared__ uint32_t ws[16];
    const uint32_t total = part_scan<uint32_t, AddU32>(job.chunk_cnt, job.chunk_base, job.n_chunks * WAVES, ws);
    if (threadIdx.x == 0) {
        const uint32_t last = job.state[ST_LAST_LF];
        const uint32_t lines = total + ((job.eof && last < job.len) ? 1u : 0u);
        job.state[ST_NTERM] = total;
        job.state[ST_N] = lines > job.cap_lines ? 0u : lines;
        job.state[ST_NSEG] = 0u;
        job.state[ST_STATUS] = lines > job.cap_lines ? (uint32_t)S_TOO_MANY_LINES : (uint32_t)S_OK;
        job.state[ST_SETTLED] = 1u;
        job.keys[K_GRAMMAR] = ~0ull;
        job.keys[K_NONSEQ] = ~0ull;
        job.keys[K_NVALUES] = 0ull;
        job.summary[SUM_CONSUMED] = job.eof ? job.len : last;
        job.summary[SUM_NLINES] = lines;
    }
}

// ---- M3 ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MB) fill_kernel(const Job job)
{
    const uint32_t n_groups = (job.len + 15u) / 16u;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t run = job.chunk_base[blockIdx.x * WAVES + wave];          // lines in front of this wave's quarter of the chunk
    for (uint32_t it = 0; it < ITER; ++it) {
        const uint32_t g = blockIdx.x * GROUPS + wave * (GROUPS / WAVES) + it * 64u + lane;
        uint32_t m = g < n_groups ? (uint32_t)job.mask16[g] : 0u;
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        uint32_t in = c;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(in, o);
            if (lane >= o) in += t;
        }
        uint32_t j = run + in - c;
        while (m) {
            const uint32_t p = g * 16u + (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            if (j < job.cap_lines) job.lend[j] = p;
            ++j;
        }
        run += wave_sum(c);
    }
}

// ---- M4 ---------------------------------------------------------------------------------------------------------------------------
struct Parsed {
    uint32_t np, tlen, roff, rlen, flags;
};

// One line text[s, e) (no '\n' inside) under the device's grammar; returns the reason it is declined for, or 0.
__device__ __forceinline__ uint32_t parse_line(const uint8_t *text, uint32_t s, uint32_t e, Parsed &out)
{
    out.np = out.tlen = out.roff = out.rlen = out.flags = 0u;
    uint32_t tabs = 0, prev = s, t[5] = {0u, 0u, 0u, 0u, 0u};
    bool empty = false;
    for (uint32_t p = s & ~7u; p < e && tabs < 10u; p += 8u) {
        const u64 x = *reinterpret_cast<const u64 *>(text + p) ^ 0x0909090909090909ull;
        u64 z = ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x | 0x7F7F7F7F7F7F7F7Full);      // 0x80 where the byte is '\t'
        if (p < s) z &= ~0ull << (8u * (s - p));
        if (e - p < 8u) z &= (1ull << (8u * (e - p))) - 1ull;
        while (z && tabs < 10u) {
            const uint32_t q = p + ((uint32_t)__builtin_ctzll(z) >> 3);
            z &= z - 1ull;
            empty = empty || q == prev;
            if (tabs < 5u) t[tabs] = q;
            ++tabs;
            prev = q + 1u;
        }
    }
    // eleven fields, none of them empty: ten tabs, and the eleventh field has a byte that is not a tab
    if (tabs < 10u || empty || prev >= e || text[prev] == 9u) return R_FIELDS;
    uint32_t u = t[0];                                             // the last '_' of the name, t[0]: none
    for (uint32_t p = t[0]; p > s; --p)
        if (text[p - 1u] == '_') { u = p - 1u; break; }
    const bool has_us = u != t[0];
    uint32_t np = 0, pos = 0;
    if (!plain_u32(text, has_us ? u + 1u : s, t[0], np)) return R_NAME_NUMBER;
    if (!plain_u32(text, t[2] + 1u, t[3], pos)) return R_POS_NUMBER;
    out.np = np;
    out.tlen = has_us ? u - s : 0u;
    out.roff = t[1] + 1u;
    out.rlen = t[2] - t[1] - 1u;
    const bool g = span_equal(text + s, out.tlen, text + out.roff, out.rlen);
    const bool mapq42 = t[4] - t[3] == 3u && text[t[3] + 1u] == '4' && text[t[3] + 2u] == '2';
    out.flags = (g ? (uint32_t)F_G : 0u) | ((g && np == pos && mapq42) ? (uint32_t)F_VALUE : 0u);
    return R_NONE;
}

__global__ void __launch_bounds__(MB) parse_kernel(const Job job)
{
    const uint32_t n = job.state[ST_N], n_terms = job.state[ST_NTERM];
    for (uint32_t i = blockIdx.x * MB + threadIdx.x; i < n; i += gridDim.x * MB) {
        Parsed r;
        const uint32_t reason = parse_line(job.text, line_start(job, i), line_end(job, i, n_terms), r);
        job.np[i] = r.np;
        job.tlen[i] = r.tlen;
        job.roff[i] = r.roff;
        job.rlen[i] = r.rlen;
        job.flags[i] = (uint8_t)r.flags;
        if (reason) atomicMin(&job.keys[K_GRAMMAR], ((u64)i << 8) | (u64)reason);
    }
}

// ---- M5 ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t map_of(uint32_t flags)
{
    // from settled a line starts a segment unless e, from unsettled unless x; behind a start the state is settled iff g
    const uint32_t behind_start = (flags & F_G) ? 0u : 1u;
    return ((flags & F_E) ? 0u : behind_start) | (((flags & F_X) ? 0u : behind_start) << 1);
}

__global__ void __launch_bounds__(MB) relate_kernel(const Job job)
{
    __shared__ uint32_t ws[WAVES];
    const uint32_t n = job.state[ST_N], n_tiles = (n + MB - 1u) / MB;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * MB + threadIdx.x;
        uint32_t map = Compose::id();
        if (i < n) {
            const uint8_t *name = job.text + line_start(job, i);
            const uint32_t tlen = job.tlen[i];
            uint32_t f = job.flags[i] & (uint32_t)(F_VALUE | F_G);
            if (i == 0u) {
                if (job.has_carry && span_equal(name, tlen, job.carry_key, job.carry_key_len)) f |= F_E;
            } else {
                if (span_equal(name, tlen, job.text + line_start(job, i - 1u), job.tlen[i - 1u])) f |= F_E;
                if (span_equal(name, tlen, job.text + job.roff[i - 1u], job.rlen[i - 1u])) f |= F_X;
            }
            job.flags[i] = (uint8_t)f;
            map = map_of(f);
        }
        uint32_t incl, total;
        (void)block_scan<uint32_t, Compose, WAVES>(map, ws, incl, total);
        if (threadIdx.x == 0) job.part[tile] = total;
    }
}

__global__ void __launch_bounds__(1024) map_part_kernel(const Job job)
{
    __shared__ uint32_t ws[16];
    const uint32_t n = job.state[ST_N];
    (void)part_scan<uint32_t, Compose>(job.part, job.part_base, (n + MB - 1u) / MB, ws);
}

__global__ void __launch_bounds__(MB) start_kernel(const Job job)
{
    __shared__ uint32_t ws[WAVES];
    const uint32_t n = job.state[ST_N], n_tiles = (n + MB - 1u) / MB;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * MB + threadIdx.x;
        const uint32_t f = i < n ? (uint32_t)job.flags[i] : 0u;
        const uint32_t map = i < n ? map_of(f) : Compose::id();
        uint32_t incl, total;
        const uint32_t front = block_scan<uint32_t, Compose, WAVES>(map, ws, incl, total);
        // the window begins settled (line 0's e is against the carried key): the maps in front of the tile, then those in front of
        // the line, applied to state 0
        const uint32_t state_in = Compose::op(job.part_base[tile], front) & 1u;
        uint32_t start = 0;
        if (i < n) {
            start = state_in ? ((f & F_X) ? 0u : 1u) : ((f & F_E) ? 0u : 1u);
            if (start) job.flags[i] = (uint8_t)(f | F_START);
            const uint32_t np = job.np[i];
            const uint32_t before = i ? job.np[i - 1u] : job.carry_position;
            if (start ? np == 0u : np <= before) atomicMin(&job.keys[K_NONSEQ], (u64)i);
            if (i == n - 1u) job.state[ST_SETTLED] = (Compose::op(job.part_base[tile], incl) & 1u) ? 0u : 1u;
        }
        uint32_t cincl, ctotal;
        (void)block_scan<uint32_t, AddU32, WAVES>(start, ws, cincl, ctotal);
        if (threadIdx.x == 0) job.part[tile] = ctotal;
    }
}

__global__ void __launch_bounds__(1024) cnt_part_kernel(const Job job)
{
    __shared__ uint32_t ws[16];
    const uint32_t n = job.state[ST_N];
    const uint32_t starts = part_scan<uint32_t, AddU32>(job.part, job.part_base, (n + MB - 1u) / MB, ws);
    if (threadIdx.x == 0) job.state[ST_NSEG] = starts + ((n && !(job.flags[0] & F_START)) ? 1u : 0u);
}

__global__ void __launch_bounds__(MB) seg_kernel(const Job job)
{
    __shared__ uint32_t ws[WAVES];
    const uint32_t n = job.state[ST_N], n_tiles = (n + MB - 1u) / MB;
    const uint32_t carried = (n && !(job.flags[0] & F_START)) ? 1u : 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * MB + threadIdx.x;
        const uint32_t start = (i < n && (job.flags[i] & F_START)) ? 1u : 0u;
        uint32_t incl, total;
        (void)block_scan<uint32_t, AddU32, WAVES>(start, ws, incl, total);
        if (i < n) {
            const uint32_t id = job.part_base[tile] + incl + carried - 1u;
            job.seg_of[i] = id;
            if (start || i == 0u) {
                Seg &s = job.segs[id];
                s.first_line = i;
                s.key_off = start ? job.roff[i] : 0u;
                s.key_len = start ? job.rlen[i] : 0u;
                s.starts = start;
                s.base = start ? job.np[i] - 1u : job.carry_position;
                s.pad_ = 0u;
            }
        }
    }
}

__global__ void __launch_bounds__(MB) segfin_kernel(const Job job)
{
    __shared__ u64 ws[WAVES];
    const uint32_t n = job.state[ST_N], n_seg = job.state[ST_NSEG], n_tiles = (n_seg + MB - 1u) / MB;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * MB + threadIdx.x;
        u64 nv = 0;
        if (k < n_seg) {
            Seg &s = job.segs[k];
            const uint32_t behind = k + 1u < n_seg ? job.segs[k + 1u].first_line : n;
            s.n_lines = behind - s.first_line;
            s.last_pos = job.np[behind - 1u];
            nv = (u64)(uint32_t)(s.last_pos - s.base);                   // (a window that is not sequential is declined as a whole)
            s.n_values = nv;
        }
        u64 incl, total;
        (void)block_scan<u64, AddU64, WAVES>(nv, ws, incl, total);
        if (threadIdx.x == 0) job.vpart[tile] = total;
    }
}

__global__ void __launch_bounds__(1024) val_part_kernel(const Job job)
{
    __shared__ u64 ws[16];
    const uint32_t n = job.state[ST_N], n_seg = job.state[ST_NSEG], n_terms = job.state[ST_NTERM];
    const u64 n_values = part_scan<u64, AddU64>(job.vpart, job.vbase, (n_seg + MB - 1u) / MB, ws);
    if (threadIdx.x != 0) return;
    // the window's outcome
    uint32_t status = job.state[ST_STATUS], reason = R_NONE;
    u64 declined = 0;
    if (status == S_OK) {
        u64 key = job.keys[K_GRAMMAR];
        // the first byte the device does not take, if it lies in a line of this window: which line
        const uint32_t hi = job.state[ST_BAD_HI], sep = job.state[ST_BAD_SEP];
        const uint32_t bad = hi > sep ? hi : sep;
        if (bad && 0xFFFFFFFFu - bad < (uint32_t)job.summary[SUM_CONSUMED]) {
            const uint32_t off = 0xFFFFFFFFu - bad;
            uint32_t lo = 0, up = n_terms;                                 // lines whose '\n' lies in front of the byte
            while (lo < up) {
                const uint32_t mid = lo + (up - lo) / 2u;
                if (job.lend[mid] < off) lo = mid + 1u; else up = mid;
            }
            const u64 k = ((u64)lo << 8) | (u64)(hi > sep ? R_NON_ASCII : R_SEPARATOR);
            if (k < key) key = k;
        }
        if (key != ~0ull) {
            status = S_DECLINED;
            reason = (uint32_t)(key & 0xFFull);
            declined = key >> 8;
        } else if (job.keys[K_NONSEQ] != ~0ull) {
            status = S_DECLINED;
            reason = R_NOT_SEQUENTIAL;
            declined = job.keys[K_NONSEQ];
        } else if (n_values > job.max_values) {
            status = S_TOO_MANY_VALUES;
        }
    }
    job.state[ST_STATUS] = status;
    job.keys[K_NVALUES] = status == S_OK ? n_values : 0ull;
    job.summary[SUM_NSEG] = status == S_OK ? n_seg : 0u;
    job.summary[SUM_NVALUES] = status == S_OK ? n_values : 0ull;
    job.summary[SUM_STATUS] = status;
    job.summary[SUM_REASON] = reason;
    job.summary[SUM_DECLINED] = declined;
    job.summary[SUM_CARRY_POS] = (status == S_OK && n) ? job.np[n - 1u] : job.carry_position;
    job.summary[SUM_CARRY_SETTLED] = (status == S_OK && n) ? job.state[ST_SETTLED] : 1u;
}

__global__ void __launch_bounds__(MB) segoff_kernel(const Job job)
{
    __shared__ u64 ws[WAVES];
    const uint32_t n_seg = job.state[ST_NSEG], n_tiles = (n_seg + MB - 1u) / MB;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * MB + threadIdx.x;
        const u64 nv = k < n_seg ? job.segs[k].n_values : 0ull;
        u64 incl, total;
        const u64 front = block_scan<u64, AddU64, WAVES>(nv, ws, incl, total);
        if (k < n_seg) job.segs[k].value_off = job.vbase[tile] + front;
    }
}

// ---- M6 ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MB) zero_kernel(const Job job)
{
    const u64 words = (job.keys[K_NVALUES] + 15ull) / 16ull;          // <= max_values rounded up to 16: the buffer's size
    for (u64 w = (u64)blockIdx.x * MB + threadIdx.x; w < words; w += (u64)gridDim.x * MB)
        *reinterpret_cast<uint4 *>(job.values + w * 16ull) = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(MB) scatter_kernel(const Job job)
{
    if (job.state[ST_STATUS] != S_OK) return;
    const uint32_t n = job.state[ST_N];
    const u64 n_values = job.keys[K_NVALUES];
    for (uint32_t i = blockIdx.x * MB + threadIdx.x; i < n; i += gridDim.x * MB) {
        const Seg &s = job.segs[job.seg_of[i]];
        const u64 at = s.value_off + (u64)(uint32_t)(job.np[i] - s.base - 1u);
        if (at < n_values) job.values[at] = (uint8_t)(job.flags[i] & F_VALUE);
    }
}

// ---- the launches behind M1, in order, on one stream ------------------------------------------------------------------------------
inline uint32_t grid_for(uint64_t items)
{
    const uint64_t blocks = (items + MB - 1) / MB;
    return (uint32_t)(blocks < 1 ? 1 : (blocks > MAX_GRID ? MAX_GRID : blocks));
}

inline void enqueue_behind_mark(const Job &job, hipStream_t st)
{
    // a line takes at least one byte of its window ('\n', or what is left at the end of the file)
    const uint64_t line_bound = (uint64_t)job.len + 1 < job.cap_lines ? (uint64_t)job.len + 1 : job.cap_lines;
    const uint32_t lines = grid_for(line_bound), tiles = lines;
    XMM_LAUNCH(chunk_scan_kernel, dim3(1), dim3(1024), st, job);
    if (job.n_chunks) XMM_LAUNCH(fill_kernel, dim3(job.n_chunks), dim3(MB), st, job);
    XMM_LAUNCH(parse_kernel, dim3(lines), dim3(MB), st, job);
    XMM_LAUNCH(relate_kernel, dim3(tiles), dim3(MB), st, job);
    XMM_LAUNCH(map_part_kernel, dim3(1), dim3(1024), st, job);
    XMM_LAUNCH(start_kernel, dim3(tiles), dim3(MB), st, job);
    XMM_LAUNCH(cnt_part_kernel, dim3(1), dim3(1024), st, job);
    XMM_LAUNCH(seg_kernel, dim3(tiles), dim3(MB), st, job);
    XMM_LAUNCH(segfin_kernel, dim3(tiles), dim3(MB), st, job);
    XMM_LAUNCH(val_part_kernel, dim3(1), dim3(1024), st, job);
    XMM_LAUNCH(segoff_kernel, dim3(tiles), dim3(MB), st, job);
    XMM_LAUNCH(zero_kernel, dim3(grid_for((job.max_values + 15) / 16)), dim3(MB), st, job);
    XMM_LAUNCH(scatter_kernel, dim3(lines), dim3(MB), st, job);
}

}  // namespace xmm
