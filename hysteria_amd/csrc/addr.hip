// addr.hip -- the request address "host:port" over batches (include/hyobfs_addr.h,
// which states the rules): split, port, IP literal; and the way back, the text of
// an address and a port.
//
// Reference: apernet/hysteria extras/outbounds/interface.go:71-77, 113-154
// (CheckUDP / WriteTo: net.SplitHostPort + parsePortUint16, AddrEx.String),
// utils.go:29-40 (tryParseIP), acl.go:79-101 (the HostInfo the ACL is given),
// ob_direct.go:298-308 (the address of a reply).
//
//   addr_parse_kernel    One wave takes kItems consecutive addresses; lane k loads item k's
//                        offset and length (coalesced) and in the end holds and stores item
//                        k's results (coalesced again).
//                        THE SPLIT, item after item by the whole wave.  An address is read 64
//                        bytes at a time, a byte per lane; ballots turn the classes ':' '['
//                        ']' '%' '.', digit, hex and "not '0'" into 64-bit masks, and
//                        wave-uniform bit operations on the masks find what
//                        net.SplitHostPort looks at (first / last ':' and ']', a '[' past
//                        byte 0) and what the port needs (only digits behind the last ':',
//                        and where its leading zeros end).  State that must survive a
//                        window is kept in wave-uniform scalars, so a host of any length up
//                        to the limit is a loop over windows and no lane walks the text.
//                        The next item's first window is loaded before the current one is
//                        worked on.  The port's value is the at most five digits behind
//                        its leading zeros, taken from the last window's register by
//                        readlane (from memory in the one case where they straddle two
//                        windows).
//                        THE LITERAL, all items at once, a lane each.  A host of at most 45
//                        bytes lies in the first window, and the masks say whether it can be
//                        a literal at all (no '%', nothing but hex digits, ':' and '.', and
//                        at least one separator; a domain name is refused there) and
//                        whether it is read as IPv4 or IPv6 (which separator comes first).
//                        Every item's first 48 bytes are kept in a row of LDS (52 bytes
//                        apart: an odd number of dwords, so the lanes' rows start in
//                        different banks).  After the wave's last split, lane k runs the
//                        rules' own parser (addr_rules.h, the code the host functions run)
//                        over row k: a short loop per lane, kItems of them side by side.
//                        (A wave-uniform parser on the scalar unit, fed by readlane, was
//                        measured first: right, but it spends a whole wave's issue slots on
//                        one item.)
//
//   addr_format_kernel   One wave takes 64 consecutive items.  Lane k writes item k's text
//                        into its row of LDS (52 bytes apart: 13 dwords, so the lanes' rows
//                        start in different banks), zero-filled.  Then the wave copies its
//                        64 output rows, which are one contiguous range, in whole aligned
//                        dwords, a dword per lane and step, taking the bytes from the LDS
//                        rows and zeros for the rest of each row; only the range's first
//                        and last dword, which it may share with the neighbouring waves,
//                        are written by bytes.
#include "salamander_device.h"

#define HY_ADDR_FN __device__ __forceinline__
#include "addr_rules.h"

namespace hyobfs {
namespace addr {

constexpr int kWaves = 4;             // waves per workgroup
constexpr int kItems = 32;            // addresses per wave of the parse kernel (at most 64: a lane each)
constexpr uint32_t kWin = 48;         // bytes of an address's first window that are kept for the literal parser
constexpr uint32_t kRow = 52;         // bytes between the format kernel's LDS rows
static_assert(kRow >= HYOBFS_ADDR_FORMAT_MAX && kRow % 4 == 0 && (kRow / 4) % 2 == 1, "dword rows, an odd pitch");
static_assert(HYOBFS_ADDR_LITERAL_MAX + 1 <= kWin && kWin <= kRow, "a host that may be a literal lies in the kept bytes");

struct ParseArgs {
    const uint8_t* src;
    const uint64_t* off;
    const uint32_t* len;                // parse_batch
    const hyobfs_udp_parsed* parsed;    // parse_udp_batch (then len is null)
    uint64_t n;
    int32_t* status;
    uint64_t* name_off;
    uint32_t* name_len;
    uint8_t* ipv4;
    uint8_t* ipv6;
    uint8_t* ip_flags;
    uint16_t* port;
};

__device__ __forceinline__ uint64_t bits_below(uint32_t b) { return b < 64 ? ~(~0ull << b) : ~0ull; }   // bits [0, b)
__device__ __forceinline__ uint32_t lane_get32(uint32_t x, uint32_t k) {   // lane k's x, k wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)k);
}
__device__ __forceinline__ uint64_t lane_get64(uint64_t x, uint32_t k) {
    const uint32_t hi = lane_get32((uint32_t)(x >> 32), k), lo = lane_get32((uint32_t)x, k);
    return (uint64_t)hi << 32 | lo;
}

// Byte sources of rule P's port_value (addr_rules.h).  LaneBytes: byte i is the register c of lane base + i
// (a window of the text, a byte per lane); MemBytes: byte i of p, which every lane loads.  Both hand out scalars.
struct LaneBytes {
    uint32_t c, base;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return lane_get32(c, base + i); }
};
struct MemBytes {
    const uint8_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return uni32(p[i]); }
};

enum { kNoLiteral = 0, kMaybeV4 = 1, kMaybeV6 = 2 };
struct Parsed {
    int32_t status;
    uint32_t host_off, host_len, port, lit;
};

// One address p[0, L), L <= HYOBFS_UDP_MAX_ADDR, by the whole wave; c0 is this lane's byte of the first
// window (0 past L).  Wave-uniform: every lane gets the same result.
__device__ __forceinline__ Parsed parse_one(const uint8_t* p, uint32_t L, uint32_t c0, uint32_t lane) {
    Parsed r{HYOBFS_OK, 0, 0, 0, kNoLiteral};
    SplitFacts f{L, kNone, kNone, kNone, kNone, false, false, false};
    bool port_bad = false;        // a byte that is no digit behind the last ':' seen so far
    uint32_t port_nz = kNone;     // the first byte that is not '0' behind it
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
            const uint64_t after = valid & ~bits_below(b + 1);
            port_bad = (after & ~digit) != 0;
            port_nz = (after & nz) ? pos + __builtin_ctzll(after & nz) : kNone;
        } else {
            port_bad |= (valid & ~digit) != 0;
            if (port_nz == kNone && (valid & nz)) port_nz = pos + __builtin_ctzll(valid & nz);
        }
        if (rb) {
            if (f.first_rb == kNone) f.first_rb = pos + __builtin_ctzll(rb);
            f.last_rb = pos + 63 - __builtin_clzll(rb);
        }
        f.lb_later |= (pos == 0 ? lb & ~1ull : lb) != 0;
    }
    // the one byte SplitHostPort reads by its position: needed only where "[...]" is not followed by the last ':'
    if (f.lb0 && f.first_rb != kNone && f.first_rb + 1 < L && f.first_rb + 1 != f.last_colon)
        f.colon_after_rb = uni32(p[f.first_rb + 1]) == ':';
    const Split s = split_decide(f);
    if (s.status != HYOBFS_OK) {
        r.status = s.status;
        return r;
    }
    // rule P: digits only, and the value of what follows the leading zeros
    const uint32_t nsig = port_nz == kNone ? 0u : L - port_nz;
    bool port_ok = s.port_len != 0 && !port_bad;
    if (port_ok && nsig) {
        if (nsig > 5) port_ok = false;
        else if (port_nz >= pos_last) port_ok = port_value(LaneBytes{c_last, port_nz - pos_last}, nsig, &r.port);
        else port_ok = port_value(MemBytes{p + port_nz}, nsig, &r.port);   // the digits straddle two windows
    }
    if (!port_ok) {
        r.status = HYOBFS_ADDR_ERR_PORT;
        r.port = 0;
        return r;
    }
    r.host_off = s.host_off;
    r.host_len = s.host_len;
    // rule I, as far as the masks decide it: can the host be a literal, and of which kind
    if (s.host_len >= 1 && s.host_len <= HYOBFS_ADDR_LITERAL_MAX) {
        const uint64_t hm = bits_below(s.host_off + s.host_len) & ~bits_below(s.host_off);
        if (!(hm & w_pct) && !(hm & ~w_lit) && (hm & w_sep))
            r.lit = ((w_dot >> __builtin_ctzll(hm & w_sep)) & 1) ? kMaybeV4 : kMaybeV6;   // '.' first: IPv4
    }
    return r;
}

__device__ __forceinline__ uint32_t first_window(const uint8_t* p, uint32_t L, uint32_t lane) {
    return lane < L ? (uint32_t)p[lane] : 0u;
}

__global__ __launch_bounds__(64 * kWaves) void addr_parse_kernel(ParseArgs A) {
    const uint32_t lane = threadIdx.x & 63, wid = uni32(threadIdx.x >> 6);
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + wid) * kItems;   // the wave's first item
    if (i0 >= A.n) return;   // whole waves
    const uint32_t cnt = uni32((uint32_t)min((uint64_t)kItems, A.n - i0));
    // lane k: item k's slice, and in the end its results
    uint64_t my_off = 0;
    uint32_t my_len = 0;
    int32_t my_st = HYOBFS_OK;
    if (lane < cnt) {
        const uint64_t i = i0 + lane;
        if (A.parsed) {
            const hyobfs_udp_parsed q = A.parsed[i];
            if (q.status != HYOBFS_OK) {
                my_st = HYOBFS_ADDR_ERR_NO_ADDR;
            } else {
                my_off = A.off[i] + q.addr_off;
                my_len = q.addr_len;
            }
        } else {
            my_off = A.off[i];
            my_len = A.len[i];
        }
        if (my_len > HYOBFS_UDP_MAX_ADDR) {   // nothing of it is read
            my_st = HYOBFS_ADDR_ERR_TOO_LONG;
            my_len = 0;
        }
    }
    __shared__ uint32_t s_rows[kWaves][kItems * kRow / 4];
    uint8_t* const rows = reinterpret_cast<uint8_t*>(s_rows[wid]);
    uint32_t r_hoff = 0, r_nlen = 0, r_port = 0, r_lit = kNoLiteral;
    uint64_t o = lane_get64(my_off, 0);
    uint32_t L = lane_get32(my_len, 0);
    uint32_t c0 = first_window(A.src + o, L, lane);
    for (uint32_t k = 0; k < cnt; ++k) {   // wave-uniform
        const uint64_t o_next = k + 1 < cnt ? lane_get64(my_off, k + 1) : 0;
        const uint32_t L_next = k + 1 < cnt ? lane_get32(my_len, k + 1) : 0;
        const uint32_t c_next = first_window(A.src + o_next, L_next, lane);   // in flight while item k is split
        if (lane_get32((uint32_t)my_st, k) == HYOBFS_OK) {
            if (lane < kWin) rows[k * kRow + lane] = (uint8_t)c0;
            const Parsed r = parse_one(A.src + o, L, c0, lane);
            if (lane == k) {
                my_st = r.status;
                if (r.status == HYOBFS_OK) {
                    r_hoff = r.host_off;
                    r_nlen = r.host_len;
                    r_port = r.port;
                    r_lit = r.lit;
                }
            }
        }
        o = o_next;
        L = L_next;
        c0 = c_next;
    }
    hy_wave_sync();   // the rows are in LDS
    // rules I and T, a lane per item
    uint64_t r_hi = 0, r_lo = 0;
    uint32_t r_flags = 0;
    if (r_lit != kNoLiteral) {
        const PtrBytes host{rows + lane * kRow + r_hoff};
        bool ok;
        if (r_lit == kMaybeV4) {
            uint32_t v4 = 0;
            ok = parse_v4(host, 0, r_nlen, &v4);
            r_lo = 0xFFFF00000000ull | v4;
        } else {
            ok = parse_v6(host, r_nlen, &r_hi, &r_lo);
        }
        if (ok) r_flags = is_v4_mapped(r_hi, r_lo) ? HYOBFS_ADDR_HAS_IPV4 : HYOBFS_ADDR_HAS_IPV6;
    }
    const uint64_t r_noff = my_st == HYOBFS_OK ? my_off + r_hoff : 0;
    if (lane >= cnt) return;
    const uint64_t i = i0 + lane;
    A.status[i] = my_st;
    A.name_off[i] = r_noff;
    A.name_len[i] = r_nlen;
    A.ip_flags[i] = (uint8_t)r_flags;
    A.port[i] = (uint16_t)r_port;
    const uint32_t v4 = (r_flags & HYOBFS_ADDR_HAS_IPV4) ? (uint32_t)r_lo : 0u;
    const uint64_t h6 = (r_flags & HYOBFS_ADDR_HAS_IPV6) ? r_hi : 0ull, l6 = (r_flags & HYOBFS_ADDR_HAS_IPV6) ? r_lo : 0ull;
    if ((reinterpret_cast<uintptr_t>(A.ipv4) & 3) == 0) {
        reinterpret_cast<uint32_t*>(A.ipv4)[i] = __builtin_bswap32(v4);
    } else {
        for (uint32_t b = 0; b < 4; ++b) A.ipv4[4 * i + b] = (uint8_t)(v4 >> (24 - 8 * b));
    }
    if ((reinterpret_cast<uintptr_t>(A.ipv6) & 7) == 0) {
        reinterpret_cast<uint64_t*>(A.ipv6)[2 * i] = __builtin_bswap64(h6);
        reinterpret_cast<uint64_t*>(A.ipv6)[2 * i + 1] = __builtin_bswap64(l6);
    } else {
        for (uint32_t b = 0; b < 8; ++b) {
            A.ipv6[16 * i + b] = (uint8_t)(h6 >> (56 - 8 * b));
            A.ipv6[16 * i + 8 + b] = (uint8_t)(l6 >> (56 - 8 * b));
        }
    }
}

// ---------------------------------------------------------------- format
struct FormatArgs {
    const uint8_t* ip;
    const uint8_t* family;
    const uint16_t* port;
    uint64_t n;
    uint8_t* out;
    uint64_t stride;
    uint64_t base_off;
    uint32_t* out_len;
    hyobfs_udp_meta* meta;
    int32_t* status;
};

__device__ __forceinline__ uint64_t load_be64(const uint8_t* p, bool aligned) {
    if (aligned) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(p));
    uint64_t v = 0;
    for (uint32_t b = 0; b < 8; ++b) v = v << 8 | p[b];
    return v;
}

// The wave's rows, `span` bytes from dst on (dst 4-aligned, the rows start vb bytes in), a dword per lane and
// step.  T: an integer type that holds span.
template <class T>
__device__ __forceinline__ void copy_rows(uint8_t* dst, uint32_t vb, T span, T stride, const uint8_t* rows, uint32_t lane) {
    const T ndw = (span + 3) / 4;
    for (T t0 = 0; t0 < ndw; t0 += 64) {   // wave-uniform
        const T t = t0 + lane;
        if (t >= ndw) continue;
        const T q = 4 * t;
        const T v0 = q < vb ? 0 : q - vb;   // the dword's first byte that belongs to the rows
        T row = v0 / stride, col = v0 - row * stride;
        uint32_t w = 0, have = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (q + j < vb || q + j >= span) continue;
            const uint32_t b = col < kRow ? rows[(uint32_t)row * kRow + (uint32_t)col] : 0u;
            w |= b << (8 * j);
            have |= 1u << j;
            if (++col == stride) {
                col = 0;
                ++row;
            }
        }
        uint8_t* const d = dst + (uint64_t)q;
        if (have == 0xF) {
            *reinterpret_cast<uint32_t*>(d) = w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (have >> j & 1) d[j] = (uint8_t)(w >> (8 * j));
        }
    }
}

__global__ __launch_bounds__(64 * kWaves) void addr_format_kernel(FormatArgs A) {
    __shared__ uint32_t s_rows[kWaves][64 * kRow / 4];
    const uint32_t lane = threadIdx.x & 63, wid = uni32(threadIdx.x >> 6);
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + wid) * 64;   // the wave's first item
    if (i0 >= A.n) return;   // whole waves
    const uint32_t cnt = uni32((uint32_t)min((uint64_t)64, A.n - i0));
    uint8_t* const rows = reinterpret_cast<uint8_t*>(s_rows[wid]);
#pragma unroll
    for (uint32_t k = 0; k < kRow / 4; ++k) s_rows[wid][lane * (kRow / 4) + k] = 0;
    if (lane < cnt) {
        const uint64_t i = i0 + lane;
        const bool al = (reinterpret_cast<uintptr_t>(A.ip) & 7) == 0;
        const uint32_t fam = A.family[i];
        uint64_t hi = load_be64(A.ip + 16 * i, al);
        const uint64_t lo = load_be64(A.ip + 16 * i + 8, al);
        if (fam == 4) hi &= 0xFFFFFFFF00000000ull;
        const int len = format(hi, lo, fam, A.port[i], rows + lane * kRow);
        A.status[i] = len < 0 ? len : HYOBFS_OK;
        A.out_len[i] = len < 0 ? 0u : (uint32_t)len;
        if (A.meta && len >= 0) {
            A.meta[i].addr_off = A.base_off + i * A.stride;
            A.meta[i].addr_len = (uint32_t)len;
        }
    }
    hy_wave_sync();   // the rows are in LDS
    uint8_t* const first = A.out + i0 * A.stride;
    const uint32_t vb = (uint32_t)(reinterpret_cast<uintptr_t>(first) & 3);
    const uint64_t span = uni64((uint64_t)vb + (uint64_t)cnt * A.stride);
    if (span < 0xFFFFFFF0ull)
        copy_rows<uint32_t>(first - vb, vb, (uint32_t)span, (uint32_t)A.stride, rows, lane);
    else
        copy_rows<uint64_t>(first - vb, vb, span, A.stride, rows, lane);
}

}  // namespace addr
}  // namespace hyobfs

using namespace hyobfs;
using namespace hyobfs::addr;

static int launch_parse(const ParseArgs& A, void* stream) {
    const uint64_t blocks = (A.n + kWaves * kItems - 1) / (kWaves * kItems);
    if (blocks > 0x7FFFFFFFull) return HYOBFS_ERR_INVALID;
    hipLaunchKernelGGL(addr_parse_kernel, dim3((uint32_t)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

extern "C" {

int hyobfs_addr_parse_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, uint64_t n, int32_t* status,
                            uint64_t* name_off, uint32_t* name_len, uint8_t* ipv4, uint8_t* ipv6, uint8_t* ip_flags,
                            uint16_t* port, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!src || !off || !len || !status || !name_off || !name_len || !ipv4 || !ipv6 || !ip_flags || !port)
        return HYOBFS_ERR_INVALID;
    return launch_parse(ParseArgs{src, off, len, nullptr, n, status, name_off, name_len, ipv4, ipv6, ip_flags, port}, stream);
}

int hyobfs_addr_parse_udp_batch(const uint8_t* in, const uint64_t* in_off, const hyobfs_udp_parsed* parsed, uint64_t n,
                                int32_t* status, uint64_t* name_off, uint32_t* name_len, uint8_t* ipv4, uint8_t* ipv6,
                                uint8_t* ip_flags, uint16_t* port, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!in || !in_off || !parsed || !status || !name_off || !name_len || !ipv4 || !ipv6 || !ip_flags || !port)
        return HYOBFS_ERR_INVALID;
    return launch_parse(ParseArgs{in, in_off, nullptr, parsed, n, status, name_off, name_len, ipv4, ipv6, ip_flags, port},
                        stream);
}

int hyobfs_addr_format_batch(const uint8_t* ip, const uint8_t* family, const uint16_t* port, uint64_t n, uint8_t* out,
                             uint64_t out_stride, uint64_t base_off, uint32_t* out_len, hyobfs_udp_meta* meta,
                             int32_t* status, void* stream) {
    if (n == 0) return HYOBFS_OK;
    if (!ip || !family || !port || !out || !out_len || !status || out_stride < HYOBFS_ADDR_FORMAT_MAX)
        return HYOBFS_ERR_INVALID;
    const uint64_t blocks = (n + kWaves * 64 - 1) / (kWaves * 64);
    if (blocks > 0x7FFFFFFFull || out_stride > (~0ull >> 8) / 64) return HYOBFS_ERR_INVALID;
    const FormatArgs A{ip, family, port, n, out, out_stride, base_off, out_len, meta, status};
    hipLaunchKernelGGL(addr_format_kernel, dim3((uint32_t)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, A);
    return hy_status(hipGetLastError());
}

}  // extern "C"
