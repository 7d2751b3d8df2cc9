// request.hip -- the request hook over batches (include/hyobfs_request.h, which
// states the rules): the TCP request framing, Sniffer.Check, the rewrite of the
// request address, and the TCP response rows.
//
// Reference: apernet/hysteria core/internal/protocol/proxy.go:32-149
// (ReadTCPRequest, WriteTCPResponse), padding.go, extras/sniff/sniff.go:67-89
// (Check), 121-125 (the rewrite), extras/utils/portunion.go:100-107 (Contains).
//
//   req_parse_kernel     A lane per stream prefix.  Rule R looks at the two varints only (at most
//                        eight bytes at the item's start and eight behind the address), so no lane
//                        walks a text; offsets, lengths and results are coalesced.
//
//   req_check_kernel     The shape of addr_parse_kernel (addr.hip).  One wave takes kItems
//                        consecutive texts; lane k loads item k's gate, offset and length and in
//                        the end stores item k's verdict.  THE SPLIT AND ATOI, item after item by
//                        the whole wave: 64 bytes a window, a byte per lane, ballots for ':' '['
//                        ']' and the digit classes; net.SplitHostPort's facts, whether anything
//                        but digits stands behind the port's first byte, and where the port's
//                        leading zeros end are wave-uniform scalars that survive a window, so a
//                        port with hundreds of zeros, or a sign or the last ':' on a window edge,
//                        is the same loop.  The port's first byte (a sign or a digit) is taken by
//                        its position afterwards.  The value is the at most 19 digits behind the
//                        zeros (readlane, or memory where they straddle two windows).  THE
//                        LITERAL (only without RewriteDomain), all items at once, a lane each,
//                        by the rules' own parser over the first window kept in LDS, as in
//                        addr.hip.  THE UNION: one bit of the port set per item.
//
//   req_rewrite_kernel   One wave takes kRItems consecutive items, lane k their metadata.  Per item
//                        the wave finds the address's last ':' and whether the name needs
//                        brackets (ballots over 64-byte windows), and then writes the row as
//                        [ '[' ] name [ ']' ] ':' port, or the address, and zeros to the row's
//                        end: whole aligned dwords, a dword per lane and step, bytes only in the
//                        row's first and last dword.
//
//   resp_build_kernel    The hot, store-bound one.  One wave takes kRItems consecutive rows, lane
//                        k computes row k's layout and stores its length and status.  Then row
//                        after row the wave writes exactly [0, out_len): a dword per lane and
//                        step, each byte chosen by its position (status, varint, message, varint,
//                        padding); a dword of padding costs one SplitMix64 step when it lies
//                        within a four-byte block of rule G and two when it straddles.  (Making
//                        such a dword at once from the blocks' 16-bit fields, without the
//                        per-byte selects, measured the same: 0.87 ms against 0.84 ms for 1M rows.)
#include "salamander_device.h"

#define HY_REQ_FN __device__ __forceinline__
#include "request_rules.h"

struct hyobfs_portset {
    int device;
    uint32_t* bits;   // 2048 words, device memory
};

namespace hyobfs {
namespace request {

using addr::is_digit;
using addr::is_hex;
using addr::PtrBytes;
using addr::Split;
using addr::SplitFacts;

constexpr int kWaves = 4;          // waves per workgroup
constexpr int kItems = 32;         // texts per wave of the check kernel (at most 64: a lane each)
constexpr int kRItems = 16;        // rows per wave of the rewrite and the response kernels
constexpr uint32_t kWin = 48;      // bytes of a text's first window kept for the literal parser
constexpr uint32_t kRow = 52;      // bytes between the LDS rows: 13 dwords, so the lanes' rows start in different banks
static_assert(HYOBFS_ADDR_LITERAL_MAX + 1 <= kWin && kWin <= kRow && kRow % 4 == 0 && (kRow / 4) % 2 == 1, "rows");
constexpr uint64_t kMaxRowStride = 0xFFFFFFF0ull;

__device__ __forceinline__ uint64_t bits_below(uint32_t b) { return b < 64 ? ~(~0ull << b) : ~0ull; }   // bits [0, b)
__device__ __forceinline__ uint32_t lane_get32(uint32_t x, uint32_t k) {   // lane k's x, k wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)k);
}
__device__ __forceinline__ uint64_t lane_get64(uint64_t x, uint32_t k) {
    const uint32_t hi = lane_get32((uint32_t)(x >> 32), k), lo = lane_get32((uint32_t)x, k);
    return (uint64_t)hi << 32 | lo;
}
struct LaneBytes {   // byte i is the register c of lane base + i
    uint32_t c, base;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return lane_get32(c, base + i); }
};
struct MemBytes {   // byte i of p, which every lane loads
    const uint8_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return uni32(p[i]); }
};

// ---------------------------------------------------------------- request parse
struct ReqParseArgs {
    const uint8_t* src;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t n;
    int32_t* status;
    uint32_t* need;
    uint64_t* addr_off;
    uint32_t* addr_len;
    uint64_t* rest_off;
    uint32_t* rest_len;
};

__global__ __launch_bounds__(64 * kWaves) void req_parse_kernel(ReqParseArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * (64 * kWaves) + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t off = A.off[i];
    const uint32_t len = A.len[i];
    const Framed f = parse_framed(PtrBytes{A.src + off}, len, 0);
    const bool ok = f.status == HYOBFS_OK;
    A.status[i] = f.status;
    A.need[i] = f.need;
    A.addr_off[i] = ok ? off + f.text_off : 0;
    A.addr_len[i] = f.text_len;
    A.rest_off[i] = ok ? off + f.consumed : 0;
    A.rest_len[i] = ok ? len - f.consumed : 0;
}

// ---------------------------------------------------------------- check
struct CheckArgs {
    const uint8_t* src;
    const uint64_t* off;
    const uint32_t* len;
    const int32_t* status_in;
    uint64_t n;
    bool rewrite_domain;
    const uint32_t* bits;   // the port set, or null
    uint8_t* check;
};

enum { kNoLiteral = 0, kMaybeV4 = 1, kMaybeV6 = 2 };
struct Checked {
    bool pass;   // C1, C2, C4 (and C3 as far as the masks decide it)
    uint32_t host_off, host_len, port16, lit;
};

// Rules C1-C5 over one text p[0, L), 0 < L <= 2048, by the whole wave; c0 is this lane's byte of the first
// window (0 past L).  Wave-uniform: every lane gets the same result.
__device__ __forceinline__ Checked check_one(const uint8_t* p, uint32_t L, uint32_t c0, uint32_t lane, bool want_literal) {
    Checked r{false, 0, 0, 0, kNoLiteral};
    if (lane_get32(c0, 0) == '@') return r;   // C1
    SplitFacts f{L, kNone, kNone, kNone, kNone, false, false, false};
    // behind the port's first byte, that is from last ':' + 2 on: a byte that is no digit, the first that is not '0'
    bool tail_bad = false;
    uint32_t tail_nz = kNone;
    uint64_t w_lit = 0, w_sep = 0, w_dot = 0, w_pct = 0;   // the first window: hex / ':' / '.', the separators, '.', '%'
    uint32_t c_last = c0, pos_last = 0;                     // the last window
    for (uint32_t pos = 0; pos < L; pos += 64) {   // L is wave-uniform
        const bool in = lane < L - pos;
        const uint32_t c = pos == 0 ? c0 : in ? p[pos + lane] : 0u;
        c_last = c;
        pos_last = pos;
        const uint64_t valid = bits_below(L - pos);
        const uint64_t colon = __ballot(c == ':'), rb = __ballot(c == ']'), lb = __ballot(c == '[');
        const uint64_t digit = __ballot(in && is_digit(c)), nz = __ballot(in && c != '0');
        if (pos == 0) {
            const uint64_t dot = __ballot(c == '.'), hex = __ballot(in && is_hex(c));
            w_pct = __ballot(c == '%');
            w_dot = dot;
            w_sep = colon | dot;
            w_lit = hex | w_sep;
            f.lb0 = lb & 1;
        }
        if (colon) {
            const uint32_t b = 63 - __builtin_clzll(colon);
            if (f.first_colon == kNone) f.first_colon = pos + __builtin_ctzll(colon);
            f.last_colon = pos + b;
            const uint64_t after = valid & ~bits_below(b + 2);
            tail_bad = (after & ~digit) != 0;
            tail_nz = (after & nz) ? pos + __builtin_ctzll(after & nz) : kNone;
        } else {
            uint64_t v = valid;
            if (f.last_colon != kNone && f.last_colon + 1 == pos) v &= ~1ull;   // the port's first byte opens this window
            tail_bad |= (v & ~digit) != 0;
            if (tail_nz == kNone && (v & nz)) tail_nz = pos + __builtin_ctzll(v & nz);
        }
        if (rb) {
            if (f.first_rb == kNone) f.first_rb = pos + __builtin_ctzll(rb);
            f.last_rb = pos + 63 - __builtin_clzll(rb);
        }
        f.lb_later |= (pos == 0 ? lb & ~1ull : lb) != 0;
    }
    if (f.lb0 && f.first_rb != kNone && f.first_rb + 1 < L && f.first_rb + 1 != f.last_colon)
        f.colon_after_rb = uni32(p[f.first_rb + 1]) == ':';
    const Split s = split_decide(f);   // C2
    if (s.status != HYOBFS_OK) return r;
    // C4: [sign] digits
    if (s.port_len == 0 || tail_bad) return r;
    const uint32_t c1 = s.port_off >= pos_last ? lane_get32(c_last, s.port_off - pos_last) : uni32(p[s.port_off]);
    const bool sign = is_sign(c1);
    if (!sign && !is_digit(c1)) return r;
    if (sign && s.port_len == 1) return r;
    const uint32_t nz_pos = (!sign && c1 != '0') ? s.port_off : tail_nz;
    const uint32_t nsig = nz_pos == kNone ? 0u : L - nz_pos;
    if (nsig > 19) return r;   // ErrRange
    bool ok = true;
    if (nsig) {
        if (nz_pos >= pos_last) ok = atoi_port16(LaneBytes{c_last, nz_pos - pos_last}, nsig, c1 == '-', &r.port16);
        else ok = atoi_port16(MemBytes{p + nz_pos}, nsig, c1 == '-', &r.port16);   // the digits straddle two windows
    }
    if (!ok) return r;
    r.host_off = s.host_off;
    r.host_len = s.host_len;
    if (want_literal) {   // C3, as far as the masks decide it: can the host be a literal, and of which kind
        if (s.host_len >= 1 && s.host_len <= HYOBFS_ADDR_LITERAL_MAX) {
            const uint64_t hm = bits_below(s.host_off + s.host_len) & ~bits_below(s.host_off);
            if (!(hm & w_pct) && !(hm & ~w_lit) && (hm & w_sep))
                r.lit = ((w_dot >> __builtin_ctzll(hm & w_sep)) & 1) ? kMaybeV4 : kMaybeV6;   // '.' first: IPv4
        }
        if (r.lit == kNoLiteral) return r;   // a domain
    }
    r.pass = true;
    return r;
}

__device__ __forceinline__ uint32_t first_window(const uint8_t* p, uint32_t L, uint32_t lane) {
    return lane < L ? (uint32_t)p[lane] : 0u;
}

__global__ __launch_bounds__(64 * kWaves) void req_check_kernel(CheckArgs A) {
    const uint32_t lane = threadIdx.x & 63, wid = uni32(threadIdx.x >> 6);
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + wid) * kItems;   // the wave's first item
    if (i0 >= A.n) return;   // whole waves
    const uint32_t cnt = uni32((uint32_t)min((uint64_t)kItems, A.n - i0));
    uint64_t my_off = 0;
    uint32_t my_len = 0;   // 0: the item is not read and its verdict is 0 (the gate, the LIMIT, the empty text)
    if (lane < cnt) {
        const uint64_t i = i0 + lane;
        if (!A.status_in || A.status_in[i] == 0) {
            my_off = A.off[i];
            my_len = A.len[i];
            if (my_len > HYOBFS_UDP_MAX_ADDR) my_len = 0;
        }
    }
    __shared__ uint32_t s_rows[kWaves][kItems * kRow / 4];
    uint8_t* const rows = reinterpret_cast<uint8_t*>(s_rows[wid]);
    const bool want_literal = !A.rewrite_domain;
    bool r_pass = false;
    uint32_t r_hoff = 0, r_hlen = 0, r_port = 0, r_lit = kNoLiteral;
    uint64_t o = lane_get64(my_off, 0);
    uint32_t L = lane_get32(my_len, 0);
    uint32_t c0 = first_window(A.src + o, L, lane);
    for (uint32_t k = 0; k < cnt; ++k) {   // wave-uniform
        const uint64_t o_next = k + 1 < cnt ? lane_get64(my_off, k + 1) : 0;
        const uint32_t L_next = k + 1 < cnt ? lane_get32(my_len, k + 1) : 0;
        const uint32_t c_next = first_window(A.src + o_next, L_next, lane);   // in flight while item k is looked at
        if (L) {
            if (want_literal && lane < kWin) rows[k * kRow + lane] = (uint8_t)c0;
            const Checked r = check_one(A.src + o, L, c0, lane, want_literal);
            if (lane == k) {
                r_pass = r.pass;
                r_hoff = r.host_off;
                r_hlen = r.host_len;
                r_port = r.port16;
                r_lit = r.lit;
            }
        }
        o = o_next;
        L = L_next;
        c0 = c_next;
    }
    hy_wave_sync();   // the rows are in LDS
    if (r_pass && want_literal) {   // C3: rule I, a lane per item
        const PtrBytes host{rows + lane * kRow + r_hoff};
        uint64_t hi = 0, lo = 0;
        uint32_t v4 = 0;
        r_pass = r_lit == kMaybeV4 ? addr::parse_v4(host, 0, r_hlen, &v4) : addr::parse_v6(host, r_hlen, &hi, &lo);
    }
    if (r_pass && A.bits) r_pass = (A.bits[r_port >> 5] >> (r_port & 31)) & 1u;   // C6, rule K
    if (lane < cnt) A.check[i0 + lane] = r_pass ? 1 : 0;
}

// ---------------------------------------------------------------- rows: dwords, bytes at the edges
// out[0, span) gets byte_at(x) for x in [0, span): whole aligned dwords, a dword per lane and step; the first
// and the last dword, which reach outside the range, are written by bytes.
template <class F>
__device__ __forceinline__ void write_range(uint8_t* out, uint32_t span, uint32_t lane, F&& byte_at) {
    const uint32_t vb = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3);
    uint8_t* const dst = out - vb;
    const uint32_t end = vb + span, ndw = (end + 3) / 4;
    for (uint32_t t0 = 0; t0 < ndw; t0 += 64) {   // wave-uniform
        const uint32_t t = t0 + lane;
        if (t >= ndw) continue;
        const uint32_t q = 4 * t;
        uint32_t w = 0, have = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (q + j < vb || q + j >= end) continue;
            w |= (byte_at(q + j - vb) & 0xFFu) << (8 * j);
            have |= 1u << j;
        }
        uint8_t* const d = dst + q;
        if (have == 0xF) {
            *reinterpret_cast<uint32_t*>(d) = w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (have >> j & 1) d[j] = (uint8_t)(w >> (8 * j));
        }
    }
}

// ---------------------------------------------------------------- rewrite
struct RewriteArgs {
    const uint8_t* src;
    const uint64_t* off;
    const uint32_t* len;
    const int32_t* status_in;
    const uint8_t* check;
    const uint8_t* names;
    uint32_t name_stride;
    const hyobfs_sniff_result* sres;
    uint64_t n;
    uint8_t* out;
    uint64_t stride;
    uint64_t base_off;
    uint64_t* row_off;
    uint32_t* out_len;
    uint8_t* rewritten;
    int32_t* status;
};

// the last position in p[0, L) whose byte is ':' (kNone for none), and whether some byte needs brackets
__device__ __forceinline__ void scan_text(const uint8_t* p, uint32_t L, uint32_t lane, uint32_t* last_colon, bool* brackets) {
    uint32_t lc = kNone;
    bool br = false;
    for (uint32_t pos = 0; pos < L; pos += 64) {   // wave-uniform
        const uint32_t c = lane < L - pos ? (uint32_t)p[pos + lane] : 0u;
        const uint64_t colon = __ballot(c == ':'), pct = __ballot(c == '%');
        if (colon) lc = pos + 63 - __builtin_clzll(colon);
        br |= (colon | pct) != 0;
    }
    *last_colon = lc;
    *brackets = br;
}

__global__ __launch_bounds__(64 * kWaves) void req_rewrite_kernel(RewriteArgs A) {
    const uint32_t lane = threadIdx.x & 63, wid = uni32(threadIdx.x >> 6);
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + wid) * kRItems;   // the wave's first item
    if (i0 >= A.n) return;   // whole waves
    const uint32_t cnt = uni32((uint32_t)min((uint64_t)kRItems, A.n - i0));
    uint64_t my_off = 0;
    uint32_t my_len = 0, my_nlen = 0, my_mode = kCopy;
    int32_t my_st = HYOBFS_OK;
    if (lane < cnt) {
        const uint64_t i = i0 + lane;
        if (A.status_in && A.status_in[i] != 0) {
            my_st = HYOBFS_REQ_ERR_NO_ADDR;   // W0
        } else {
            my_off = A.off[i];
            my_len = A.len[i];
            const bool chk = A.check[i] != 0;
            if (chk) {
                const hyobfs_sniff_result sr = A.sres[i];
                my_mode = rewrite_mode(true, sr.status, sr.name_len);
                my_nlen = sr.name_len;
            }
            if (my_mode == kLeftToHost) my_st = HYOBFS_REQ_ERR_HOST;
        }
    }
    uint32_t my_total = 0, my_rew = 0;
    for (uint32_t k = 0; k < cnt; ++k) {   // wave-uniform
        int32_t st = (int32_t)lane_get32((uint32_t)my_st, k);
        const uint32_t mode = lane_get32(my_mode, k), L = lane_get32(my_len, k), nlen = lane_get32(my_nlen, k);
        const uint8_t* const p = A.src + lane_get64(my_off, k);
        const uint8_t* const name = A.names + (i0 + k) * (uint64_t)A.name_stride;
        // the row is [pre '['] seg1 [mid: "]:" or ":"] seg2, then zeros
        const uint8_t *seg1 = p, *seg2 = p;
        uint32_t pre = 0, len1 = 0, mid = 0, len2 = 0;
        if (st == HYOBFS_OK && mode == kJoin) {
            uint32_t lc, unused_lc;
            bool br, unused_br;
            scan_text(p, L, lane, &lc, &unused_br);
            scan_text(name, nlen, lane, &unused_lc, &br);
            if (lc == kNone) {
                st = HYOBFS_ADDR_ERR_MISSING_PORT;
            } else {
                pre = br ? 1 : 0;
                seg1 = name;
                len1 = nlen;
                mid = 1 + pre;
                seg2 = p + lc + 1;
                len2 = L - lc - 1;
            }
        } else if (st == HYOBFS_OK) {
            len1 = L;
        }
        const uint64_t total = (uint64_t)pre + len1 + mid + len2;
        const bool cap = total > A.stride;
        if (cap) st = HYOBFS_REQ_ERR_CAP;
        if (lane == k) {
            my_st = st;
            my_total = st == HYOBFS_OK || cap ? (uint32_t)total : 0u;
            my_rew = st == HYOBFS_OK && mode == kJoin;
        }
        if (cap) continue;   // nothing of the row is written
        if (st != HYOBFS_OK) pre = len1 = mid = len2 = 0;
        write_range(A.out + (i0 + k) * A.stride, (uint32_t)A.stride, lane, [&](uint32_t x) -> uint32_t {
            if (x < pre) return '[';
            x -= pre;
            if (x < len1) return seg1[x];
            x -= len1;
            if (x < mid) return mid == 2 && x == 0 ? ']' : ':';
            x -= mid;
            return x < len2 ? (uint32_t)seg2[x] : 0u;
        });
    }
    if (lane >= cnt) return;
    const uint64_t i = i0 + lane;
    A.status[i] = my_st;
    A.out_len[i] = my_total;
    A.rewritten[i] = (uint8_t)my_rew;
    A.row_off[i] = A.base_off + i * A.stride;
}

// ---------------------------------------------------------------- response build
struct RespArgs {
    const uint8_t* ok;
    const uint32_t* msg_idx;
    const uint8_t* msgs;
    const uint64_t* msg_off;
    const uint32_t* msg_len;
    uint32_t n_msgs;
    const uint32_t* pad_len;
    uint64_t seed;
    uint64_t n;
    uint8_t* out;
    uint64_t stride;
    uint32_t* out_len;
    int32_t* status;
};

__global__ __launch_bounds__(64 * kWaves) void resp_build_kernel(RespArgs A) {
    const uint32_t lane = threadIdx.x & 63, wid = uni32(threadIdx.x >> 6);
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + wid) * kRItems;   // the wave's first row
    if (i0 >= A.n) return;   // whole waves
    const uint32_t cnt = uni32((uint32_t)min((uint64_t)kRItems, A.n - i0));
    uint64_t my_moff = 0;
    uint32_t my_mlen = 0, my_plen = 0, my_ok = 0, my_total = 0;   // my_total: the bytes to write, 0 for a row that is not OK
    if (lane < cnt) {
        const uint64_t i = i0 + lane;
        const uint32_t m = A.msg_idx[i];
        int32_t st = HYOBFS_OK;
        uint32_t olen = 0;
        if (m >= A.n_msgs) {
            st = HYOBFS_ERR_INVALID;
        } else {
            my_moff = A.msg_off[m];
            my_mlen = A.msg_len[m];
            my_plen = A.pad_len[i];
            my_ok = A.ok[i];
            const uint64_t total = frame_layout(1, my_mlen, my_plen).total();
            olen = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
            if (total > A.stride) st = HYOBFS_REQ_ERR_CAP;
            else my_total = (uint32_t)total;   // the stride is below 2^32
        }
        A.status[i] = st;
        A.out_len[i] = olen;
    }
    for (uint32_t k = 0; k < cnt; ++k) {   // wave-uniform
        const uint32_t total = lane_get32(my_total, k);
        if (total == 0) continue;
        const uint32_t mlen = lane_get32(my_mlen, k), plen = lane_get32(my_plen, k);
        const uint32_t first = lane_get32(my_ok, k) ? 0u : 1u;
        const uint8_t* const msg = A.msgs + lane_get64(my_moff, k);
        const FrameLayout f = frame_layout(1, mlen, plen);
        const uint32_t text_at = (uint32_t)f.text_at(), padlen_at = (uint32_t)f.padlen_at(), pad_at = (uint32_t)f.pad_at();
        const uint64_t state = pad_state(A.seed, i0 + k);
        uint64_t z = 0;
        uint32_t z_blk = kNone;   // the block of rule G that z is
        write_range(A.out + (i0 + k) * A.stride, total, lane, [&](uint32_t x) -> uint32_t {
            if (x >= pad_at) {
                const uint32_t pk = x - pad_at;
                if ((pk >> 2) != z_blk) {
                    z_blk = pk >> 2;
                    z = pad_block(state, pk);
                }
                return pad_char((uint32_t)(z >> (16 * (pk & 3))) & 0xFFFFu);
            }
            if (x >= padlen_at) return varint_byte(plen, f.vl_pad, x - padlen_at);
            if (x >= text_at) return msg[x - text_at];
            return x == 0 ? first : (uint32_t)varint_byte(mlen, f.vl_text, x - 1);
        });
    }
}

}  // namespace request
}  // namespace hyobfs

using namespace hyobfs;
using namespace hyobfs::request;

static bool grid_for(uint64_t n, uint64_t per_block, uint32_t* blocks) {
    const uint64_t b = (n + per_block - 1) / per_block;
    *blocks = (uint32_t)b;
    return b <= 0x7FFFFFFFull;
}

extern "C" {

int hyobfs_portset_new(const hyobfs_port_range* ranges, uint32_t n_ranges, int device, hyobfs_portset** set) {
    if (!set || (!ranges && n_ranges)) return HYOBFS_ERR_INVALID;
    *set = nullptr;
    uint32_t* const bits = static_cast<uint32_t*>(calloc(2048, 4));
    if (!bits) return HYOBFS_ERR_NOMEM;
    for (uint32_t r = 0; r < n_ranges; ++r)
        for (uint32_t p = ranges[r].start; p <= ranges[r].end; ++p) bits[p >> 5] |= 1u << (p & 31);
    int count = 0, prev = -1;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        free(bits);
        return HYOBFS_ERR_NO_DEVICE;
    }
    auto* s = static_cast<hyobfs_portset*>(malloc(sizeof(hyobfs_portset)));
    if (!s) {
        free(bits);
        return HYOBFS_ERR_NOMEM;
    }
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipError_t e = hipSetDevice(device);
    void* mem = nullptr;
    if (e == hipSuccess) e = hipMalloc(&mem, 2048 * 4);
    if (e == hipSuccess) e = hipMemcpy(mem, bits, 2048 * 4, hipMemcpyHostToDevice);
    if (prev >= 0) (void)hipSetDevice(prev);
    free(bits);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        free(s);
        return e == hipErrorOutOfMemory ? HYOBFS_ERR_NOMEM : HYOBFS_ERR_HIP;
    }
    s->device = device;
    s->bits = static_cast<uint32_t*>(mem);
    *set = s;
    return HYOBFS_OK;
}

void hyobfs_portset_free(hyobfs_portset* set) {
    if (!set) return;
    if (set->bits) (void)hipFree(set->bits);
    free(set);
}

int hyobfs_tcp_request_parse_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, uint64_t n,
                                   int32_t* status, uint32_t* need, uint64_t* addr_off, uint32_t* addr_len,
                                   uint64_t* rest_off, uint32_t* rest_len, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!src || !off || !len || !status || !need || !addr_off || !addr_len || !rest_off || !rest_len)
        return HYOBFS_ERR_INVALID;
    uint32_t blocks;
    if (!grid_for(n, 64 * kWaves, &blocks)) return HYOBFS_ERR_INVALID;
    const ReqParseArgs A{src, off, len, n, status, need, addr_off, addr_len, rest_off, rest_len};
    hipLaunchKernelGGL(req_parse_kernel, dim3(blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

int hyobfs_sniff_check_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const int32_t* status_in,
                             uint64_t n, int is_udp, int rewrite_domain, const hyobfs_portset* portset, uint8_t* check,
                             void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!src || !off || !len || !check || (is_udp != 0 && is_udp != 1)) return HYOBFS_ERR_INVALID;
    uint32_t blocks;
    if (!grid_for(n, kWaves * kItems, &blocks)) return HYOBFS_ERR_INVALID;
    const CheckArgs A{src, off, len, status_in, n, rewrite_domain != 0, portset ? portset->bits : nullptr, check};
    hipLaunchKernelGGL(req_check_kernel, dim3(blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

int hyobfs_request_rewrite_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, const int32_t* status_in,
                                 const uint8_t* check, const uint8_t* names, uint32_t name_stride,
                                 const hyobfs_sniff_result* sres, uint64_t n, uint8_t* out, uint64_t out_stride,
                                 uint64_t base_off, uint64_t* row_off, uint32_t* out_len, uint8_t* rewritten,
                                 int32_t* status, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!src || !off || !len || !check || !names || !sres || !out || !row_off || !out_len || !rewritten || !status ||
        out_stride == 0 || out_stride > kMaxRowStride)
        return HYOBFS_ERR_INVALID;
    uint32_t blocks;
    if (!grid_for(n, kWaves * kRItems, &blocks)) return HYOBFS_ERR_INVALID;
    const RewriteArgs A{src, off, len, status_in, check, names, name_stride, sres, n, out, out_stride, base_off,
                        row_off, out_len, rewritten, status};
    hipLaunchKernelGGL(req_rewrite_kernel, dim3(blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

int hyobfs_tcp_response_build_batch(const uint8_t* ok, const uint32_t* msg_idx, const uint8_t* msgs,
                                    const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n_msgs,
                                    const uint32_t* pad_len, uint64_t seed, uint64_t n, uint8_t* out, uint64_t out_stride,
                                    uint32_t* out_len, int32_t* status, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!ok || !msg_idx || !pad_len || !out || !out_len || !status || (n_msgs && (!msgs || !msg_off || !msg_len)) ||
        out_stride > kMaxRowStride)
        return HYOBFS_ERR_INVALID;
    uint32_t blocks;
    if (!grid_for(n, kWaves * kRItems, &blocks)) return HYOBFS_ERR_INVALID;
    const RespArgs A{ok, msg_idx, msgs, msg_off, msg_len, n_msgs, pad_len, seed, n, out, out_stride, out_len, status};
    hipLaunchKernelGGL(resp_build_kernel, dim3(blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

}  // extern "C"
